"""The XCD-local tile walk of the persistent Doppler kernels at nD <= 513 (blah2_amd/csrc/doppler_walk.hpp): it changes
no operation and no order inside a tile, so the maps and the metrics of a launch must have the SAME BITS whatever grid
walks it.  Grids divisible by 8 take the new walk (ragged
last iterations, walks that cross CPI boundaries, labels whose range ends inside a CPI); grid 5, and a launch that has
fewer tiles than the forced grid, keep the strided one.  Every run also passes the oracle gates of
tests/test_timed_kernels_gpu.py (the fp64 reference of a case is computed once and shared by its grids)."""
import functools

import numpy as np
import pytest

from oracle import blah2_oracle as O

from test_timed_kernels_gpu import CFG2, assert_cpi, b2  # noqa: F401  (b2 is a fixture)

pytestmark = pytest.mark.gpu

G513 = (-7, 292, -256, 256, 1_026_000, 1_026_000)  # 513 x 300: 19 tiles per CPI, the last one of 12 columns
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)  # 201 x 111: 7 whole / 14 half tiles per CPI, both ragged
TARGETS = ((37, -13.0, 0.05),)


@functools.lru_cache(maxsize=None)
def _case(geom, seeds):
    """Inputs and fp64 references of a case; read-only for every test that shares them."""
    dmin, dmax, fmin, fmax, fs, n = geom
    xs, ys = zip(*(O.synth_iq(n, seed=s, fs=fs, targets=TARGETS, quantise=True) for s in seeds))
    d = O.ambiguity_dims(dmin, dmax, fmin, fmax, fs, n, True)
    refs = [O.ambiguity_process(d, x, y) for x, y in zip(xs, ys)]
    x = np.stack(xs).astype(np.complex64)
    y = np.stack(ys).astype(np.complex64)
    for a in (x, y, *refs):
        a.setflags(write=False)
    return d, x, y, refs


def run_grid(b2, geom, seeds, kernel, grid):
    """The CPIs of a case through one blah2hip_amb_process_dev call on a forced Doppler grid -> (maps, metrics, grid that
    ran, tiles); every CPI against the oracle."""
    import torch
    from blah2_amd import _lib
    d, xh, yh, refs = _case(geom, tuple(seeds))
    B, n = len(refs), geom[5]
    amb = b2.Ambiguity(*geom, True, max_batch=B)
    amb.set_doppler_kernel(kernel)
    amb.set_doppler_grid(grid)
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    assert (d.n_doppler_bins, d.n_delay_bins) == (nD, nC)
    out = torch.zeros((B, nD, nC), dtype=torch.complex64, device="cuda")
    met = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
    x, y = torch.tensor(xh).cuda(), torch.tensor(yh).cuda()  # copies: the shared arrays are read-only
    amb.process_dev(b2.FMT_C32, x.data_ptr(), y.data_ptr(), B, n, out.data_ptr(), met.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert amb.last_doppler_kernel() == kernel
    ran, tiles = amb.info(_lib.INFO_DOPPLER_GRID), amb.info(_lib.INFO_DOPPLER_TILES)
    amb.close()
    o, m = out.cpu().numpy(), met.cpu().numpy()
    for c in range(B):
        assert_cpi(o[c], m[c], refs[c], f"cpi {c} of {B} [{kernel}, grid {grid}]")
    return o, m, ran, tiles


def assert_same_bits(a, b, tag):
    for c in range(len(a[0])):
        assert np.array_equal(a[0][c].view(np.uint64), b[0][c].view(np.uint64)), f"{tag}: map of cpi {c}"
        assert np.array_equal(a[1][c].view(np.uint64), b[1][c].view(np.uint64)), f"{tag}: metrics of cpi {c}"


@pytest.fixture(scope="module")
def g513_on_grid5(b2):
    o, m, ran, tiles = run_grid(b2, G513, (640, 641, 642), "pfa513", 5)
    assert (ran, tiles) == (5, 57)
    return o, m


@pytest.mark.parametrize("grid", [8, 16, 24, 56])
def test_pfa513_bits_do_not_depend_on_the_walk(b2, g513_on_grid5, grid):
    """57 tiles (3 CPIs x 19, last tile of 12 columns): 8 labels of ceil(57/8) = 8 tiles, the last label one short, on
    1, 2, 3 and 7 workgroups per label -- 8, 4, 3 and 2 iterations, the last ones ragged, labels crossing CPI boundaries."""
    o, m, ran, tiles = run_grid(b2, G513, (640, 641, 642), "pfa513", grid)
    assert (ran, tiles) == (grid, 57)
    assert_same_bits((o, m), g513_on_grid5, f"grid {grid} against grid 5")


def test_pfa513_fewer_tiles_than_the_forced_grid(b2):
    """One CPI on a forced grid of 24: the launch has 19 workgroups, no multiple of 8 -> the strided walk, one tile each."""
    seeds = (640,)
    o, m, ran, tiles = run_grid(b2, G513, seeds, "pfa513", 24)
    assert (ran, tiles) == (19, 19)
    o5, m5, ran5, _ = run_grid(b2, G513, seeds, "pfa513", 5)
    assert ran5 == 5
    assert_same_bits((o, m), (o5, m5), "19 workgroups against grid 5")


def test_pfa513_configs1_geometry(b2):
    """411 columns: rows of 3288 bytes (every row piece straddles two lines), a last tile of 11 columns; 2 CPIs = 52 tiles
    on 16 workgroups (labels of 7 tiles on 2 slots: 4 iterations, the last ragged) against grid 5."""
    seeds = (650, 651)
    o, m, ran, tiles = run_grid(b2, CFG2, seeds, "pfa513", 16)
    assert (ran, tiles) == (16, 52)
    o5, m5, ran5, _ = run_grid(b2, CFG2, seeds, "pfa513", 5)
    assert ran5 == 5
    assert_same_bits((o, m), (o5, m5), "grid 16 against grid 5")


@pytest.mark.parametrize("kernel,tiles_per_cpi", [("tile16", 7), ("tile8", 14), ("tile16wg", 7), ("tile8k", 14)])
def test_chirp_z_tile_kernels_bits_do_not_depend_on_the_walk(b2, kernel, tiles_per_cpi):
    """doppler_tile1k_kernel<16|8> and doppler_tile_kernel<16|8> on 201 x 111, 8 CPIs: 56 / 112 tiles on grids 8 and 16
    against grid 5."""
    seeds = tuple(range(660, 668))
    o5, m5, ran5, tiles = run_grid(b2, SMALL, seeds, kernel, 5)
    assert (ran5, tiles) == (5, 8 * tiles_per_cpi)
    for grid in (8, 16):
        o, m, ran, _ = run_grid(b2, SMALL, seeds, kernel, grid)
        assert ran == grid
        assert_same_bits((o, m), (o5, m5), f"{kernel}: grid {grid} against grid 5")
