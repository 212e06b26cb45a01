"""GPU: the array in the sample domain -- the covariance of the channels' samples (blah2hip_amb_sample_covariance_dev:
sample_cov_kernel + cov_fold_kernel) and beam planes formed from them (blah2hip_amb_beam_samples_dev / _wdev:
beam_samples_kernel, beam_samples_wdev_kernel), through the C ABI like tests/test_adaptive_beam_gpu.py.

No reference counterpart; the checks are the fp64 NumPy restatements of tests/samples_beam_crafted.py with derived bounds,
and the oracle's map for the chain.  Every output has guard words behind it (beam planes: in every gap between n_samples
and beam_stride too).

Bounds
  * covariance, int8 planes: EXACT equality with the int64 sum (every product <= 2^14, every sum < 2^53).
  * covariance, fp32 planes: |R_dev - R_fp64| <= 4 * 2^-24 * sum |y_i| |y_j| per entry (blah2hip_amb_covariance_dev's contract).
  * beam planes: per sample |y_dev - y_fp64| <= 4 (K + 1) * 2^-24 * sum_k |w_k| |y_k|: per component 2K fused multiply-adds,
    each rounding at most 2^-24 of a partial sum that sum_k |w_k| |y_k| bounds; compared with <=, so an all-zero sample must
    come out 0.
  * weights: tests/test_adaptive_beam_gpu.py's bound, 2^-23 ||w||inf + 64 K 2^-53 cond(R_l) ||w||inf, cond(R_l) <= 1e5 asserted.
  * the chain: tests/gates.py (map_cell_gate 1e-4, db_map_gate 0.005 dB) and metrics within 1e-3 dB, against the oracle's map
    of the fp64 beam formed with the device's own weights read back.
Geometries: 100 000 samples per CPI and 100 001 (heads and tails of the wide accesses); planes at equal and at different
offsets modulo 16 bytes (wide and single-sample kernels); odd strides, so that the offset changes from CPI to CPI.
"""
import ctypes as C

import numpy as np
import pytest

import samples_beam_crafted as S
from gates import db_map_gate, map_cell_gate

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 24
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


# ---- planes ---------------------------------------------------------------------------------------------------------------
def in_planes(torch, fmt_i8, ys, stride, offsets):
    """ys [K, n_cpi, n] complex64 or [K, n_cpi, n, 2] int8 -> (keep-alive tensors, pointers): plane k starts ``offsets[k]``
    samples into a 16-byte aligned buffer, CPI c at c * stride samples; the gaps hold a value (77) that a read beyond a CPI
    would pick up."""
    keep, ptrs = [], []
    K, n_cpi, n = ys.shape[:3]
    for k in range(K):
        if fmt_i8:
            host = np.full((offsets[k] + n_cpi * stride, 2), 77, dtype=np.int8)
        else:
            host = np.full((offsets[k] + n_cpi * stride,), 77 + 77j, dtype=np.complex64)
        for c in range(n_cpi):
            host[offsets[k] + c * stride:offsets[k] + c * stride + n] = ys[k, c]
        t = torch.from_numpy(host).cuda()
        assert t.data_ptr() % 16 == 0
        keep.append(t)
        ptrs.append(t.data_ptr() + offsets[k] * (2 if fmt_i8 else 8))
    return keep, ptrs


class BeamPlanes:
    """n_beams guarded complex64 planes of n_cpi CPIs, beam_stride apart, plane b ``offsets[b]`` samples into its buffer."""

    def __init__(self, torch, n_beams, n_cpi, n, stride, offsets):
        self.n_cpi, self.n, self.stride, self.offsets = n_cpi, n, stride, offsets
        self.whole = [torch.full((2 * (offsets[b] + n_cpi * stride) + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
                      for b in range(n_beams)]
        for w in self.whole:
            assert w.data_ptr() % 16 == 0
        self.ptrs = [w.data_ptr() + 8 * offsets[b] for b, w in enumerate(self.whole)]

    def read(self):
        """(planes [n_beams, n_cpi, n] complex64, True where every word outside them still holds the guard pattern)"""
        out, clean = [], True
        for b, w in enumerate(self.whole):
            words = w.cpu().numpy().view(np.uint32)
            body = words[2 * self.offsets[b]:2 * (self.offsets[b] + self.n_cpi * self.stride)].reshape(self.n_cpi, self.stride, 2)
            clean = clean and bool((words[:2 * self.offsets[b]] == GUARD).all()) and bool((body[:, self.n:] == GUARD).all())
            clean = clean and bool((words[2 * (self.offsets[b] + self.n_cpi * self.stride):] == GUARD).all())
            out.append(np.ascontiguousarray(body[:, :self.n]).view(np.float32).view(np.complex64)[..., 0])
        return np.stack(out), clean

    def untouched(self):
        return all(bool((w.cpu().numpy().view(np.uint32) == GUARD).all()) for w in self.whole)


def offsets_for(kind, count, fmt_i8):
    """'same': every plane at a 16-byte boundary.  'mixed': offsets that differ modulo 16 bytes from plane to plane."""
    if kind == "same":
        return [0] * count
    steps = (1, 0, 3, 2, 5, 1, 7, 4) if fmt_i8 else (1, 0, 1, 1, 0, 1, 0, 0)
    return [steps[k] for k in range(count)]


def random_planes(K, n_cpi, n, seed, fmt_i8, scaled=False):
    rng = np.random.default_rng(seed)
    if fmt_i8:
        return rng.integers(-128, 128, size=(K, n_cpi, n, 2), dtype=np.int64).astype(np.int8)  # every value of int8, -128 included
    z = (rng.standard_normal((K, n_cpi, n)) + 1j * rng.standard_normal((K, n_cpi, n))) * np.sqrt(0.5)
    if scaled:
        z *= (10.0 ** np.arange(K))[:, None, None]  # a dropped or swapped channel shows
    z = z.astype(np.complex64)
    assert (z.real != 0).all() and (z.imag != 0).all()
    return z


def as_c128(ys, fmt_i8):
    return S.as_complex(ys) if fmt_i8 else ys.astype(np.complex128)


def cov_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, window=None):
    K = len(ptrs)
    wc, cov = guarded(torch, (n_cpi, K, K), torch.complex128)
    amb.sample_covariance_dev(b2.FMT_I8 if fmt_i8 else b2.FMT_C32, ptrs, n_cpi, stride, cov.data_ptr(), window, stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(wc)
    R = cov.cpu().numpy()
    assert np.array_equal(R, np.conj(np.swapaxes(R, -1, -2)))  # both triangles, exact conjugates
    assert (R[:, np.arange(K), np.arange(K)].imag == 0).all()
    return R


# ---- 1. covariance, int8: exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_int8_covariance_is_exact(b2, torch, K):
    n_cpi = 3
    for geom, kind in ((S.GEOM, "same"), (S.GEOM_ODD, "same"), (S.GEOM_ODD, "mixed")):
        amb = handle(b2, geom)
        n = geom[5]
        stride = n + 37 if n % 2 == 0 else n + 36  # odd: the offset modulo the access changes from CPI to CPI
        assert stride % 2 == 1 and amb.get_n_samples() == n
        yq = random_planes(K, n_cpi, n, seed=100 + K, fmt_i8=True)
        keep, ptrs = in_planes(torch, True, yq, stride, offsets_for(kind, K, True))
        for window in (None, (1, n - 1), (4711, 4712), (3, 3 + 777)):  # all, [1, n-1), one sample, odd start and odd length
            R = cov_dev(b2, torch, amb, True, ptrs, n_cpi, stride, window)
            want = S.covariance_int(yq, *(window or (0, None)))
            assert np.array_equal(R.real, want[..., 0].astype(np.float64)) and np.array_equal(R.imag, want[..., 1].astype(np.float64)), (geom, kind, window)
            R2 = cov_dev(b2, torch, amb, True, ptrs, n_cpi, stride, window)
            assert np.array_equal(R.view(np.uint64), R2.view(np.uint64))  # two calls: the same bits


# ---- 2. covariance, fp32 planes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fp32_covariance_is_within_its_bound(b2, torch, K):
    n_cpi = 3
    worst = 0.0
    for geom, kind in ((S.GEOM, "same"), (S.GEOM_ODD, "same"), (S.GEOM_ODD, "mixed")):
        amb = handle(b2, geom)
        n = geom[5]
        stride = n + 37 if n % 2 == 0 else n + 36
        ys = random_planes(K, n_cpi, n, seed=200 + K, fmt_i8=False, scaled=True)
        keep, ptrs = in_planes(torch, False, ys, stride, offsets_for(kind, K, False))
        for window in (None, (1, n - 1), (4711, 4712), (3, 3 + 777)):
            R = cov_dev(b2, torch, amb, False, ptrs, n_cpi, stride, window)
            s0, s1 = window or (0, None)
            ref = S.sample_covariance(ys, s0, s1)
            a = np.abs(ys.astype(np.complex128))[..., s0:s1]
            bound = 4 * EPS32 * np.einsum("icn,jcn->cij", a, a)
            err = np.abs(R - ref)
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(R.view(np.float64)).all() and (err <= bound).all(), (geom, kind, window, float((err / bound).max()))
            assert np.array_equal(R.view(np.uint64), cov_dev(b2, torch, amb, False, ptrs, n_cpi, stride, window).view(np.uint64))
    print(f"fp32 sample covariance K={K}: largest error / bound {worst:.3e}")


# ---- 3. beam planes -------------------------------------------------------------------------------------------------------
def weights(n_cpi, n_beams, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_cpi, n_beams, K)) + 1j * rng.standard_normal((n_cpi, n_beams, K))).astype(np.complex64)


def beams_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, w, n, beam_stride, kind, wdev=False):
    """w: [n_beams, K] (host weights) or [n_cpi, n_beams, K] with wdev.  -> planes [n_beams, n_cpi, n] complex64"""
    nb = w.shape[-2]
    out = BeamPlanes(torch, nb, n_cpi, n, beam_stride, offsets_for(kind, nb, False))
    fmt = b2.FMT_I8 if fmt_i8 else b2.FMT_C32
    if wdev:
        d_w = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        amb.beam_samples_wdev(fmt, ptrs, n_cpi, stride, d_w.data_ptr(), out.ptrs, beam_stride, stream(torch))
    else:
        amb.beam_samples_dev(fmt, ptrs, n_cpi, stride, w, out.ptrs, beam_stride, stream(torch))
    torch.cuda.synchronize()
    got, clean = out.read()
    assert clean, "a word outside the n_samples of a CPI was written"
    return got


@pytest.mark.parametrize("fmt_i8", [False, True], ids=["fp32", "int8"])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_beam_planes_are_within_their_bound(b2, torch, K, fmt_i8):
    worst = 0.0
    base = random_planes(K, 3, S.GEOM_ODD[5], seed=300 + K, fmt_i8=fmt_i8, scaled=not fmt_i8)
    if fmt_i8:
        base[:, :, 5] = 0  # an all-zero sample has bound 0 and must come out 0
    for geom, kind in ((S.GEOM, "same"), (S.GEOM_ODD, "same"), (S.GEOM_ODD, "mixed")):
        amb = handle(b2, geom)
        n = geom[5]
        stride, beam_stride = (n + 37, n + 5) if n % 2 == 0 else (n + 36, n + 4)  # both odd, and different
        assert stride % 2 == 1 and beam_stride % 2 == 1
        for n_cpi in (1, 3):
            ys = np.ascontiguousarray(base[:, :n_cpi, :n])
            keep, ptrs = in_planes(torch, fmt_i8, ys, stride, offsets_for(kind, K, fmt_i8))
            y128 = as_c128(ys, fmt_i8)
            for nb in (1, 3, 8):
                w = weights(n_cpi, nb, K, seed=17 + 10 * K + nb)
                got = beams_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, w[0], n, beam_stride, kind)
                ref = S.beam_samples(y128, w[0].astype(np.complex128))
                bound = 4 * (K + 1) * EPS32 * np.einsum("bk,kcn->bcn", np.abs(w[0].astype(np.complex128)), np.abs(y128))
                err = np.abs(got.astype(np.complex128) - ref)
                assert (err <= bound).all(), (geom, kind, n_cpi, nb, float((err / np.maximum(bound, 1e-300)).max()))
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
                # the same weights in every CPI from the device: the same bits
                rep = beams_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, np.repeat(w[:1], n_cpi, axis=0), n, beam_stride, kind, wdev=True)
                assert np.array_equal(rep.view(np.uint32), got.view(np.uint32)), (geom, kind, n_cpi, nb)
                if n_cpi > 1 and nb == 3:  # a set per CPI: each CPI matches the call with its own weights
                    per = beams_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, w, n, beam_stride, kind, wdev=True)
                    for c in range(n_cpi):
                        one = got if c == 0 else beams_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, w[c], n, beam_stride, kind)
                        assert np.array_equal(per[:, c].view(np.uint32), one[:, c].view(np.uint32)), (geom, kind, nb, c)
    print(f"beam planes K={K} int8={fmt_i8}: largest error / bound {worst:.3e}")


@pytest.mark.parametrize("fmt_i8", [False, True], ids=["fp32", "int8"])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_permutation_weights_copy_the_planes(b2, torch, K, fmt_i8):
    n_cpi = 3
    perm = np.random.default_rng(K).permutation(K)
    w = np.zeros((K, K), dtype=np.complex64)
    w[np.arange(K), perm] = 1.0
    for geom, kind in ((S.GEOM, "same"), (S.GEOM_ODD, "mixed")):
        amb = handle(b2, geom)
        n = geom[5]
        stride, beam_stride = (n + 37, n + 5) if n % 2 == 0 else (n + 36, n + 4)
        ys = random_planes(K, n_cpi, n, seed=400 + K, fmt_i8=fmt_i8)
        keep, ptrs = in_planes(torch, fmt_i8, ys, stride, offsets_for(kind, K, fmt_i8))
        got = beams_dev(b2, torch, amb, fmt_i8, ptrs, n_cpi, stride, w, n, beam_stride, kind)
        if fmt_i8:
            assert np.array_equal(got, S.as_complex(ys)[perm].astype(np.complex64)), (geom, kind)  # the exact conversion
        else:
            assert np.array_equal(got.view(np.uint32), ys[perm].view(np.uint32)), (geom, kind)  # bit for bit


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(b2, torch):
    from blah2_amd import _lib
    amb = handle(b2, S.GEOM)
    L, h = amb._L, amb._h
    n = S.GEOM[5]
    stride = n + 37
    K, nb, n_cpi = 2, 2, 3
    VP = C.c_void_p
    i8 = torch.zeros((8, n_cpi * stride + 8, 2), dtype=torch.int8, device="cuda")
    c32 = torch.zeros((8, n_cpi * stride + 8), dtype=torch.complex64, device="cuda")
    out = BeamPlanes(torch, 8, n_cpi, n, stride, [0] * 8)
    wc, cov = guarded(torch, (MAX_BATCH, 8, 8), torch.complex128)
    wh = np.ascontiguousarray(np.ones((8, 8)), dtype=np.complex64)
    d_w = torch.ones((MAX_BATCH, 8, 8), dtype=torch.complex64, device="cuda")

    def arr(ptrs):
        return (VP * 8)(*(list(ptrs) + [None] * (8 - len(ptrs))))

    p8 = [i8[k].data_ptr() for k in range(8)]
    p32 = [c32[k].data_ptr() for k in range(8)]
    span = ((n_cpi - 1) * stride + n)

    # covariance: (fmt, d_y, n_surv, n_cpi, cpi_stride, s0, s1, d_cov)
    good = [_lib.FMT_I8, arr(p8), K, n_cpi, stride, 0, n, cov.data_ptr()]
    bad = {
        "NULL plane array": ({1: None}, _lib.ERR_INVALID), "NULL plane": ({1: arr([p8[0], None])}, _lib.ERR_INVALID),
        "NULL output": ({7: None}, _lib.ERR_INVALID), "n_surv 0": ({2: 0}, _lib.ERR_INVALID), "n_surv 9": ({2: 9, 3: 1}, _lib.ERR_INVALID),
        "n_cpi 0": ({3: 0}, _lib.ERR_INVALID), "n_surv * n_cpi above max_batch": ({2: 8, 3: 4}, _lib.ERR_INVALID),
        "s0 == s1": ({5: 9, 6: 9}, _lib.ERR_INVALID), "s0 > s1": ({5: 10, 6: 9}, _lib.ERR_INVALID), "s1 > n_samples": ({6: n + 1}, _lib.ERR_INVALID),
        "stride below n_samples": ({4: n - 1}, _lib.ERR_INVALID), "an int8 plane at an odd address": ({1: arr([p8[0], p8[1] + 1])}, _lib.ERR_INVALID),
        "an fp32 plane off 8 bytes": ({0: _lib.FMT_C32, 1: arr([p32[0], p32[1] + 4])}, _lib.ERR_INVALID),
        "output inside an input plane": ({0: _lib.FMT_C32, 1: arr(p32), 7: p32[1] + 8 * (span - 1)}, _lib.ERR_INVALID),
        "FMT_I16": ({0: _lib.FMT_I16}, _lib.ERR_UNSUPPORTED), "FMT_F16": ({0: _lib.FMT_F16}, _lib.ERR_UNSUPPORTED),
        "FMT_I8X_C32Y": ({0: _lib.FMT_I8X_C32Y}, _lib.ERR_UNSUPPORTED), "an unknown format": ({0: 99}, _lib.ERR_UNSUPPORTED),
    }
    for name, (change, code) in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_sample_covariance_dev(h, *args, None) == code, name
    assert L.blah2hip_amb_sample_covariance_dev(None, *good, None) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(wc)
    assert L.blah2hip_amb_sample_covariance_dev(h, *good, None) == _lib.OK
    good1 = list(good)
    good1[3], good1[4] = 1, 0  # a lone CPI: any stride
    assert L.blah2hip_amb_sample_covariance_dev(h, *good1, None) == _lib.OK
    torch.cuda.synchronize()
    assert guard_intact(wc) and not untouched(wc)

    # beam planes: (fmt, d_y, n_surv, n_cpi, cpi_stride, w / d_w, n_beams, d_beam, beam_stride)
    for fn, wts in ((L.blah2hip_amb_beam_samples_dev, VP(wh.ctypes.data)), (L.blah2hip_amb_beam_samples_wdev, VP(d_w.data_ptr()))):
        good = [_lib.FMT_C32, arr(p32), K, n_cpi, stride, wts, nb, arr(out.ptrs), stride]
        bad = {
            "NULL plane array": ({1: None}, _lib.ERR_INVALID), "NULL plane": ({1: arr([p32[0], None])}, _lib.ERR_INVALID),
            "NULL weights": ({5: None}, _lib.ERR_INVALID), "NULL output array": ({7: None}, _lib.ERR_INVALID),
            "NULL beam plane": ({7: arr([out.ptrs[0], None])}, _lib.ERR_INVALID),
            "n_surv 0": ({2: 0}, _lib.ERR_INVALID), "n_surv 9": ({2: 9}, _lib.ERR_INVALID), "n_beams 0": ({6: 0}, _lib.ERR_INVALID),
            "n_beams 9": ({6: 9}, _lib.ERR_INVALID), "n_cpi 0": ({3: 0}, _lib.ERR_INVALID),
            "cpi_stride below n_samples": ({4: n - 1}, _lib.ERR_INVALID), "beam_stride below n_samples": ({8: n - 1}, _lib.ERR_INVALID),
            "an int8 plane at an odd address": ({0: _lib.FMT_I8, 1: arr([p8[0] + 1, p8[1]])}, _lib.ERR_INVALID),
            "an fp32 plane off 8 bytes": ({1: arr([p32[0] + 4, p32[1]])}, _lib.ERR_INVALID),
            "a beam plane inside an input plane": ({7: arr([out.ptrs[0], p32[1] + 8 * (span - 1)])}, _lib.ERR_INVALID),
            "a beam plane around an input plane's start": ({1: arr([p32[0], out.ptrs[1] + 8 * (span - 1)])}, _lib.ERR_INVALID),
            "a beam plane that is an input plane": ({7: arr([p32[0], out.ptrs[1]])}, _lib.ERR_INVALID),
            "two beam planes that overlap": ({7: arr([out.ptrs[0], out.ptrs[0] + 8 * (span - 1)])}, _lib.ERR_INVALID),
            "the same beam plane twice": ({7: arr([out.ptrs[0], out.ptrs[0]])}, _lib.ERR_INVALID),
            "FMT_I16": ({0: _lib.FMT_I16}, _lib.ERR_UNSUPPORTED), "FMT_F16": ({0: _lib.FMT_F16}, _lib.ERR_UNSUPPORTED),
            "FMT_I16X_C32Y": ({0: _lib.FMT_I16X_C32Y}, _lib.ERR_UNSUPPORTED), "an unknown format": ({0: -1}, _lib.ERR_UNSUPPORTED),
        }
        for name, (change, code) in bad.items():
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert fn(h, *args, None) == code, name
        assert fn(None, *good, None) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert out.untouched()
        assert bool((c32 == 0).all()) and bool((i8 == 0).all())  # the refused calls that named an input plane as an output wrote nothing
    assert L.blah2hip_amb_beam_samples_dev(h, *good[:5], VP(wh.ctypes.data), *good[6:], None) == _lib.OK
    torch.cuda.synchronize()
    got, clean = out.read()
    assert clean and (got[:nb] == 0).all() and not out.untouched()


# ---- 5. the chain, stage by stage, on the scene ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {i8: S.batch(i8) for i8 in (False, True)}


def run_map(b2, torch, amb, fmt, d_x, d_y, n_cpi, stride):
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    wm, out = guarded(torch, (n_cpi, nD, nC), torch.complex64)
    wk, met = guarded(torch, (n_cpi, 2), torch.float64)
    amb.process_dev(fmt, d_x, d_y, n_cpi, stride, out.data_ptr(), met.data_ptr(), stream(torch))
    torch.cuda.synchronize()
    assert guard_intact(wm) and guard_intact(wk)
    return out.cpu().numpy(), met.cpu().numpy()


def gate_map(tag, got, met, x128, beam128):
    """One CPI's device map and metrics against the oracle's map of the fp64 beam."""
    from oracle import blah2_oracle as O
    ref = S.oracle_map(x128, beam128)
    noise, peak = O.map_metrics(ref)
    cell = map_cell_gate(got, ref)
    db = db_map_gate(got, met[0], ref)
    print(f"{tag}: cell_rel_above_mean {cell['cell_rel_above_mean']:.3e} peak_rel {cell['peak_rel']:.3e} db_max_shown {db['db_max_shown']:.3e} "
          f"noise diff {abs(met[0] - noise):.3e} dB peak diff {abs(met[1] - peak):.3e} dB")
    assert cell["ok"], (tag, cell)
    assert db["ok"], (tag, db)
    assert abs(met[0] - noise) <= DB_TOL and abs(met[1] - peak) <= DB_TOL, tag
    return ref


@pytest.mark.parametrize("fmt_i8", [False, True], ids=["fp32", "int8"])
def test_the_adaptive_chain_stage_by_stage(b2, torch, scenes, fmt_i8):
    x, ys = scenes[fmt_i8]
    n_cpi, n, K = len(S.SEEDS), S.GEOM[5], S.K
    stride = n + 37
    amb = handle(b2, S.GEOM)
    st = stream(torch)
    fmt = b2.FMT_I8 if fmt_i8 else b2.FMT_C32
    keep, ptrs = in_planes(torch, fmt_i8, ys, stride, [0] * K)
    keepx, px = in_planes(torch, fmt_i8, x[None], stride, [0])
    x128, y128 = as_c128(x, fmt_i8), as_c128(ys, fmt_i8)
    steer32 = S.steer().astype(np.complex64)

    wc, cov = guarded(torch, (n_cpi, K, K), torch.complex128)
    ww, w = guarded(torch, (n_cpi, 1, K), torch.complex64)
    wk, ok = guarded(torch, (n_cpi,), torch.int32)
    beam = BeamPlanes(torch, 1, n_cpi, n, stride, [0])
    amb.adaptive_beam_samples_dev(fmt, ptrs, n_cpi, stride, steer32, S.LOADING, cov.data_ptr(), w.data_ptr(), ok.data_ptr(), beam.ptrs, stride,
                                  None, st)
    torch.cuda.synchronize()
    assert guard_intact(wc) and guard_intact(ww) and guard_intact(wk)

    # (a) the covariance
    R = cov.cpu().numpy()
    assert np.array_equal(R, np.conj(np.swapaxes(R, -1, -2)))
    if fmt_i8:
        want = S.covariance_int(ys)
        assert np.array_equal(R.real, want[..., 0].astype(np.float64)) and np.array_equal(R.imag, want[..., 1].astype(np.float64))
    else:
        a = np.abs(y128)
        err, bound = np.abs(R - S.sample_covariance(ys)), 4 * EPS32 * np.einsum("icn,jcn->cij", a, a)
        print(f"chain covariance: largest error / bound {float((err / bound).max()):.3e}")
        assert (err <= bound).all()

    # (b) the weights, against mvdr_weights on the device's own matrix
    w_dev = w.cpu().numpy()
    assert ok.cpu().numpy().tolist() == [1] * n_cpi
    ref_w, ok_ref = b2.mvdr_weights(R, steer32, S.LOADING)
    assert ok_ref.tolist() == [1] * n_cpi
    for c in range(n_cpi):
        cond = S.loaded_cond(R[c])
        assert cond <= S.COND_MAX, cond
        top = np.abs(ref_w[c, 0]).max()
        bound = 2.0 ** -23 * top + 64 * K * EPS64 * cond * top
        err = np.abs(w_dev[c, 0].astype(np.complex128) - ref_w[c, 0]).max()
        print(f"chain weights, CPI {c}: cond(R_l) {cond:.3e}, error / bound {err / bound:.3f}")
        assert err <= bound, (c, err, bound)

    # (c) the beam plane through the map stage, against the oracle's map of the fp64 beam with the device's weights
    got_beam, clean = beam.read()
    assert clean
    beam128 = S.beam_samples(y128, w_dev.astype(np.complex128))[0]
    bound = 4 * (K + 1) * EPS32 * np.einsum("ck,kcn->cn", np.abs(w_dev[:, 0].astype(np.complex128)), np.abs(y128))
    assert (np.abs(got_beam[0].astype(np.complex128) - beam128) <= bound).all()
    map_fmt = b2.FMT_I8X_C32Y if fmt_i8 else b2.FMT_C32
    maps, met = run_map(b2, torch, amb, map_fmt, px[0], beam.ptrs[0], n_cpi, stride)
    for c in range(n_cpi):
        gate_map(f"MVDR beam map int8={fmt_i8} CPI {c}", maps[c], met[c], x128[c], beam128[c])
        # (d) structure: the adaptive beam's map peaks at the target
        assert S.peak_cell(maps[c]) == S.TARGET_CELL, (c, S.peak_cell(maps[c]))

    # (d) ... and the conventional beam's at the direct path
    conv = BeamPlanes(torch, 1, n_cpi, n, stride, [0])
    amb.beam_samples_dev(fmt, ptrs, n_cpi, stride, S.conventional(), conv.ptrs, stride, st)
    cmaps, _ = run_map(b2, torch, amb, map_fmt, px[0], conv.ptrs[0], n_cpi, stride)
    assert conv.read()[1]
    for c in range(n_cpi):
        assert S.peak_cell(cmaps[c]) == S.DIRECT_CELL, (c, S.peak_cell(cmaps[c]))


# ---- 6. cross-check with the map domain -----------------------------------------------------------------------------------
def test_the_beam_plane_and_the_beamformed_maps_both_match_the_oracle(b2, torch, scenes):
    """Random weights, K = 4: the map of the beam plane and beamform_dev of the four channel maps, each against the oracle's
    map of the fp64 beam.  The two device maps are not compared with each other: their roundings differ."""
    x, ys = scenes[False]
    n_cpi, n, K = len(S.SEEDS), S.GEOM[5], S.K
    stride = n + 37
    amb = handle(b2, S.GEOM)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    st = stream(torch)
    keep, ptrs = in_planes(torch, False, ys, stride, [0] * K)
    keepx, px = in_planes(torch, False, x[None], stride, [0])
    w = weights(1, 1, K, seed=61)[0]
    x128, y128 = x.astype(np.complex128), ys.astype(np.complex128)
    beam128 = S.beam_samples(y128, w.astype(np.complex128))[0]

    beam = BeamPlanes(torch, 1, n_cpi, n, stride, [0])
    amb.beam_samples_dev(b2.FMT_C32, ptrs, n_cpi, stride, w, beam.ptrs, stride, st)
    maps, met = run_map(b2, torch, amb, b2.FMT_C32, px[0], beam.ptrs[0], n_cpi, stride)
    assert beam.read()[1]

    wm, chan = guarded(torch, (K, n_cpi, nD, nC), torch.complex64)
    wk, cmet = guarded(torch, (K, n_cpi, 2), torch.float64)
    wb, bmap = guarded(torch, (1, n_cpi, nD, nC), torch.complex64)
    wl, bmet = guarded(torch, (1, n_cpi, 2), torch.float64)
    amb.process_multi_dev(b2.FMT_C32, px[0], ptrs, n_cpi, stride, chan.data_ptr(), cmet.data_ptr(), st)
    amb.beamform_dev(chan.data_ptr(), K, n_cpi, w, bmap.data_ptr(), bmet.data_ptr(), st)
    torch.cuda.synchronize()
    for whole in (wm, wk, wb, wl):
        assert guard_intact(whole)
    bmaps = bmap.cpu().numpy()[0]
    for c in range(n_cpi):
        ref = S.oracle_map(x128[c], beam128[c])
        a, b = map_cell_gate(maps[c], ref), map_cell_gate(bmaps[c], ref)
        print(f"CPI {c}: beam plane's map cell_rel {a['cell_rel_above_mean']:.3e} peak_rel {a['peak_rel']:.3e}; "
              f"beamformed maps cell_rel {b['cell_rel_above_mean']:.3e} peak_rel {b['peak_rel']:.3e}")
        assert a["ok"], (c, a)
        assert b["ok"], (c, b)
