"""doppler_pfa513_kernel (BLAH2HIP_DOP_PFA513): the Doppler stage at nD = 513 on the 27 x 19 prime-factor transform,
forced, every CPI against the fp64 oracle at the gates of tests/test_timed_kernels_gpu.py and oracle/gates.py: the
configs[1] geometry (411 delay bins: a ragged last tile of 11 columns), asymmetric Doppler limits, a forced small grid
(each workgroup walks >= 3 tiles across CPI boundaries), a strong echo that takes the hot-column rewrite, and the
bits of a CPI at every batch position and across runs."""
import numpy as np
import pytest
from gates import map_cell_gate
from oracle import blah2_oracle as O

from test_hot_columns_gpu import echo_cpi
from test_timed_kernels_gpu import CFG2, b2, run_batch  # noqa: F401  (b2 is a fixture)

pytestmark = pytest.mark.gpu

G513 = (-7, 292, -256, 256, 1_026_000, 1_026_000)  # 300 delay bins: 19 tiles per CPI, the last one of 12 columns


def test_cfg2_batch(b2):
    amb = run_batch(b2, CFG2, 8, "pfa513", seeds=range(600, 608), db_gate=True)
    assert (amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (513, 411)


def test_auto_takes_it_on_full_launches(b2):
    """AUTO runs it at nD = 513 once a launch has a whole tile for each of two workgroups per CU."""
    from blah2_amd import _lib
    amb = b2.Ambiguity(*CFG2, True)
    ncu = amb.info(_lib.INFO_NUM_CU)
    amb.close()
    B = -(-2 * ncu // 26)  # 26 tiles per CPI
    run_batch(b2, CFG2, B, "auto", seeds=range(700, 700 + B), expect="pfa513")


def test_asymmetric_doppler_limits(b2):
    geom = (-10, 300, -200, 312, 1_000_000, 1_000_000)
    amb = run_batch(b2, geom, 3, "pfa513", seeds=(610, 611, 612), targets=((37, 150.0, 0.05), (90, -120.0, 0.03)))
    assert amb.get_n_doppler_bins() == 513


@pytest.mark.parametrize("grid", [4, 5])
def test_forced_small_grid(b2, grid):
    from blah2_amd import _lib
    amb = run_batch(b2, G513, 3, "pfa513", seeds=(620, 621, 622), targets=((37, -13.0, 0.05),), doppler_grid=grid)
    g, tiles = amb.info(_lib.INFO_DOPPLER_GRID), amb.info(_lib.INFO_DOPPLER_TILES)
    assert g == grid and tiles == 3 * 19 and tiles >= 3 * grid and tiles % grid != 0


def test_strong_echo_takes_the_hot_column_rewrite(b2):
    args, echo = CFG2, (37, -63.0)
    x, y = echo_cpi(args[5], args[4], 11, *echo)
    d = O.ambiguity_dims(*args, True)
    ref = O.ambiguity_process(d, x.astype(np.complex128), y.astype(np.complex128))
    amb = b2.Ambiguity(*args, True)
    amb.set_doppler_kernel("pfa513")
    amb.set_hot_columns("auto")
    got = amb.process(x, y).data.copy()
    assert amb.last_doppler_kernel() == "pfa513"
    assert (amb.hot_columns(), amb.hot_columns_missed()) == (1, 0)
    amb.close()
    g = map_cell_gate(got, ref)
    assert g["ok"] and g["cell_rel_above_mean"] <= 3e-5, g
    col = int(np.argmin(np.abs(d.delay - echo[0])))
    row = int(np.argmin(np.abs(d.doppler - echo[1])))
    assert abs(got[row, col] - ref[row, col]) <= 2e-6 * abs(ref[row, col])


def test_bits_do_not_depend_on_batch_position_or_run(b2):
    import torch
    B = 6
    amb = b2.Ambiguity(*CFG2, True, max_batch=B)
    amb.set_doppler_kernel("pfa513")
    x, y = O.synth_iq(CFG2[5], seed=630, fs=CFG2[4], targets=((37, -63.0, 0.05),), quantise=True)
    xs = torch.from_numpy(np.stack([x] * B).astype(np.complex64)).cuda()
    ys = torch.from_numpy(np.stack([y] * B).astype(np.complex64)).cuda()
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        out = torch.zeros((B, nD, nC), dtype=torch.complex64, device="cuda")
        met = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        amb.process_dev(b2.FMT_C32, xs.data_ptr(), ys.data_ptr(), B, CFG2[5], out.data_ptr(), met.data_ptr(), st)
        torch.cuda.synchronize()
        assert amb.last_doppler_kernel() == "pfa513"
        runs.append((out.cpu().numpy(), met.cpu().numpy()))
    amb.close()
    o0, m0 = runs[0]
    for o, m in runs:
        for c in range(B):
            assert np.array_equal(o[c].view(np.uint64), o0[0].view(np.uint64)), f"cpi {c}"
            assert np.array_equal(m[c], m0[0]), f"metrics of cpi {c}"
