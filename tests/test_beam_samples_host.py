"""CPU: the fp64 models of the sample-domain beams (blah2_amd.sample_covariance, blah2_amd.beam_samples) and the scene of
tests/samples_beam_crafted.py, which tests/test_beam_samples_gpu.py holds the device against."""
import numpy as np
import pytest

import samples_beam_crafted as S
from blah2_amd import beam_samples, mvdr_weights, sample_covariance


@pytest.fixture(scope="module")
def cpi():
    return S.scene(S.SEEDS[0])


def test_sample_covariance_is_the_direct_sum():
    rng = np.random.default_rng(1)
    ys = (rng.standard_normal((3, 2, 50)) + 1j * rng.standard_normal((3, 2, 50))).astype(np.complex64)
    for s0, s1 in ((0, None), (1, 49), (7, 8), (3, 30)):
        R = sample_covariance(ys, s0, s1)
        assert R.shape == (2, 3, 3)
        for c in range(2):
            for i in range(3):
                for j in range(3):
                    want = sum(complex(ys[i, c, n]) * np.conj(complex(ys[j, c, n])) for n in range(s0, 50 if s1 is None else s1))
                    assert abs(R[c, i, j] - want) <= 1e-12 * abs(want) + 1e-12, (s0, s1, c, i, j)
        assert np.allclose(R, np.conj(np.swapaxes(R, -1, -2)), rtol=0, atol=1e-12)
    assert sample_covariance(ys[:, 0]).shape == (3, 3)


def test_beam_samples_is_the_direct_sum():
    rng = np.random.default_rng(2)
    ys = (rng.standard_normal((3, 2, 40)) + 1j * rng.standard_normal((3, 2, 40))).astype(np.complex64)
    w = rng.standard_normal((2, 3)) + 1j * rng.standard_normal((2, 3))
    out = beam_samples(ys, w)
    assert out.shape == (2, 2, 40)
    wc = rng.standard_normal((2, 2, 3)) + 1j * rng.standard_normal((2, 2, 3))
    per = beam_samples(ys, wc)
    for b in range(2):
        for c in range(2):
            for n in range(40):
                want = sum(w[b, k] * complex(ys[k, c, n]) for k in range(3))
                assert abs(out[b, c, n] - want) <= 1e-13 * (1 + abs(want))
                want = sum(wc[c, b, k] * complex(ys[k, c, n]) for k in range(3))
                assert abs(per[b, c, n] - want) <= 1e-13 * (1 + abs(want))
    assert np.array_equal(beam_samples(ys, np.eye(3)), ys.astype(np.complex128))


def test_int8_covariance_in_integers_equals_the_fp64_model_exactly(cpi):
    x, ys = cpi
    _, yq = S.quantise(x, ys)
    for s0, s1 in ((0, None), (1, yq.shape[1] - 1), (4711, 4712), (3, 3 + 777)):
        Ri = S.covariance_int(yq, s0, s1)
        assert np.abs(Ri).max() < 2 ** 53
        Rf = sample_covariance(S.as_complex(yq), s0, s1)
        assert np.array_equal(Rf.real, Ri[..., 0].astype(np.float64)) and np.array_equal(Rf.imag, Ri[..., 1].astype(np.float64))
        assert (np.diagonal(Ri[..., 1]) == 0).all() and np.array_equal(Ri[..., 0], Ri[..., 0].T) and np.array_equal(Ri[..., 1], -Ri[..., 1].T)


def test_the_map_is_linear_in_the_surveillance_channel(cpi):
    x, ys = cpi
    rng = np.random.default_rng(3)
    w = rng.standard_normal((1, S.K)) + 1j * rng.standard_normal((1, S.K))
    direct = S.oracle_map(x, beam_samples(ys, w)[0])
    summed = sum(w[0, k] * S.oracle_map(x, ys[k]) for k in range(S.K))
    assert np.abs(direct - summed).max() <= 1e-13 * np.abs(direct).max()


@pytest.mark.parametrize("i8", [False, True], ids=["fp32", "int8"])
def test_the_conventional_beam_sees_the_direct_path_and_the_mvdr_beam_the_target(i8):
    for seed in S.SEEDS:
        x, ys = S.scene(seed)
        if i8:
            xq, yq = S.quantise(x, ys)
            x, ys = S.as_complex(xq), S.as_complex(yq)
        R = sample_covariance(ys)
        cond = S.loaded_cond(R)
        assert cond <= S.COND_MAX, cond
        w, ok = mvdr_weights(R, S.steer(), S.LOADING)
        assert int(ok) == 1 and abs(w[0] @ S.steer()[0] - 1.0) <= 1e-12
        assert S.peak_cell(S.oracle_map(x, beam_samples(ys, S.conventional())[0])) == S.DIRECT_CELL
        assert S.peak_cell(S.oracle_map(x, beam_samples(ys, w)[0])) == S.TARGET_CELL
        print(f"seed {seed} int8={i8}: cond(R_l) {cond:.3e}")
