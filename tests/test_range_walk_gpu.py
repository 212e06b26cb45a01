"""GPU: the ticketed pulse walk of rangew1k_kernel (blah2_amd/csrc/range_walk.hpp, BLAH2HIP_OPT_RANGE_WALK) against the
static walk.  A pulse's result does not depend on the wave that computes it, so every comparison here is on BITS: the maps
and the metrics of a ticketed launch equal those of the static launch at the same grid and at the natural grid.  The
range kernel is forced to BLAH2HIP_RANGE_WAVE1K throughout and asserted.

Shapes: the smallest at which the walk can go wrong -- grids below, at and above the eight heads (1, 3, 8, 9, 16; a forced
grid is capped at one workgroup per 12 pulses, as for the static walk), launches with fewer pulses than waves, fewer than
12 pulses in all, one segment per pulse (the ticket is then requested a whole pulse ahead), and the headline's own
instantiation (configs[1]: SHORTX, OUT7, carried y' registers) on two CPIs, whose first and last CPI also go against the
fp64 oracle by the gates of tests/gates.py.

The output buffers are filled with a NaN pattern before every call: a pulse no wave took would leave it in the map."""
import numpy as np
import pytest

from gates import db_map_gate, map_cell_gate
from oracle import blah2_oracle as O
from test_timed_kernels_gpu import CFG2, DB_TOL, PEAK_TOL

pytestmark = pytest.mark.gpu

SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)  # 21 pulses per CPI, 111 lags, 6 segments at F = 1024
FEW = (-10, 400, -2, 2, 20_000, 20_000)            # 5 pulses per CPI: two CPIs are 10 pulses, fewer than one workgroup's waves
ONE_SEG = (-10, 100, -2, 2, 3_004, 3_004)          # nCorr = 600 <= 1024 - 111 + 1: one segment per pulse, 5 pulses per CPI
GUARD = np.uint32(0x7FC0BEEF)
_inputs = {}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


def inputs(geom, n_cpi):
    """(xs, ys): int16-valued CPIs (exact in both wire formats), computed once per geometry."""
    key = (geom, n_cpi)
    if key not in _inputs:
        fs, n = geom[4], geom[5]
        _inputs[key] = tuple(zip(*(O.synth_iq(n, seed=900 + s, fs=fs, targets=((37, -13.0, 0.05),), quantise=True) for s in range(n_cpi))))
    return _inputs[key]


def upload(b2, fmt, xs, ys):
    import torch
    if fmt == "FMT_C32":
        x = torch.from_numpy(np.stack(xs).astype(np.complex64)).cuda()
        y = torch.from_numpy(np.stack(ys).astype(np.complex64)).cuda()
        return (x, y), x.data_ptr(), y.data_ptr()
    iq = np.stack([np.stack([x_.real, x_.imag, y_.real, y_.imag], axis=-1) for x_, y_ in zip(xs, ys)]).astype(np.int16)
    d = torch.from_numpy(iq).cuda()
    return (d,), d.data_ptr(), 0


def engine(b2, geom, max_batch, walk, grid):
    from blah2_amd import _lib
    amb = b2.Ambiguity(*geom, True, max_batch=max_batch)
    amb.set_fft_len(1024)
    amb.set_range_kernel(_lib.RANGE_WAVE1K)
    amb.set_range_walk(walk)
    if grid:
        amb.set_range_grid(grid)
    return amb


def call(b2, amb, fmt, dev, n_cpi, n):
    """One process call into freshly poisoned buffers: (map bits, metrics bits, map, metrics)."""
    import torch
    from blah2_amd import _lib
    keep, px, py = dev
    nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
    out = torch.full((n_cpi * nD * nC * 2,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    met = torch.full((n_cpi * 2 * 2,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    amb.process_dev(getattr(b2, fmt), px, py, n_cpi, n, out.data_ptr(), met.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert amb.info(_lib.INFO_LAST_RANGE_KERNEL) == _lib.RANGE_WAVE1K
    o, m = out.cpu().numpy().view(np.uint32), met.cpu().numpy().view(np.uint32)
    assert not (o == GUARD).any(), "a cell of the map was never written"
    return o, m, o.view(np.complex64).reshape(n_cpi, nD, nC), m.view(np.float64).reshape(n_cpi, 2)


def assert_same_bits(a, b, tag):
    assert np.array_equal(a[0], b[0]), f"{tag}: {int((a[0] != b[0]).sum())} words of the maps differ"
    assert np.array_equal(a[1], b[1]), f"{tag}: the metrics differ"


def walks_agree(b2, geom, fmt, n_cpi, grids):
    """Ticketed against static at every grid of ``grids`` (0 = the natural one), and every launch against the static walk
    at the natural grid.  Returns the natural static result."""
    from blah2_amd import _lib
    xs, ys = inputs(geom, n_cpi)
    dev = upload(b2, fmt, xs, ys)
    n = geom[5]
    base = None
    for grid in (0,) + tuple(g for g in grids if g):
        res = {}
        for walk in ("static", "ticket"):
            amb = engine(b2, geom, n_cpi, walk, grid)
            res[walk] = call(b2, amb, fmt, dev, n_cpi, n)
            used = amb.info(_lib.INFO_RANGE_GRID)
            if grid:
                assert used == grid
            amb.close()
        if base is None:
            base = res["static"]
        print(f"\n[{fmt} grid {grid or 'natural'} ({used})] static / ticket compared")
        assert_same_bits(res["ticket"], res["static"], f"{fmt} grid {grid}: ticket against static")
        assert_same_bits(res["ticket"], base, f"{fmt} grid {grid}: ticket against the static walk at the natural grid")
    return base


@pytest.mark.parametrize("fmt", ["FMT_C32", "FMT_I16"])
def test_ticketed_walk_keeps_the_bits(b2, fmt):
    """`small` x 3 CPIs (63 pulses, 6 segments each) at grids 1, 3, 8, 9, 16 and the natural one."""
    amb = engine(b2, SMALL, 3, "static", 0)
    assert (amb.dims.fft_len, amb.get_n_doppler_bins(), amb.get_n_delay_bins()) == (1024, 21, 111) and amb.dims.n_seg > 2
    amb.close()
    walks_agree(b2, SMALL, fmt, 3, (1, 3, 8, 9, 16))


def test_three_calls_on_one_handle_reset_themselves(b2):
    """n_cpi = 3, 1, 3 on one ticketed handle: the launch in the middle has fewer pulses (21) than waves (24), so waves
    leave without a pulse; every launch must find the counters at zero, and the third result is the first's, bit for bit.
    The same calls on a static handle give the same bits."""
    xs, ys = inputs(SMALL, 3)
    dev = upload(b2, "FMT_C32", xs, ys)
    n = SMALL[5]
    got = {}
    for walk in ("static", "ticket"):
        amb = engine(b2, SMALL, 3, walk, 0)
        got[walk] = [call(b2, amb, "FMT_C32", dev, k, n) for k in (3, 1, 3)]
        amb.close()
    t = got["ticket"]
    assert_same_bits(t[2], t[0], "third call against the first")
    nD, nC = 21, 111
    assert np.array_equal(t[1][0], t[0][0][:nD * nC * 2]), "the lone CPI is the first CPI of the batch"
    for k in range(3):
        assert_same_bits(t[k], got["static"][k], f"call {k}: ticket against static")


@pytest.mark.parametrize("geom,n_cpi,n_seg,grids", [(FEW, 2, None, (1,)), (ONE_SEG, 3, 1, (1, 2))], ids=["ten-pulses", "one-segment"])
def test_special_geometries(b2, geom, n_cpi, n_seg, grids):
    """Fewer than 12 pulses in all (one workgroup, two of its waves without a pulse, all eight heads searched at the end),
    and one segment per pulse (every iteration is a pulse's last; on one workgroup the 12 waves walk 15 pulses)."""
    amb = engine(b2, geom, n_cpi, "ticket", 0)
    pulses = n_cpi * amb.get_n_doppler_bins()
    if n_seg is None:
        assert pulses < 12
    else:
        assert amb.dims.n_seg == n_seg and pulses > 12
    amb.close()
    walks_agree(b2, geom, "FMT_C32", n_cpi, grids)


def test_headline_instantiation(b2):
    """configs[1] (7 segments of 576 samples, 411 lags: SHORTX, OUT7, REUSE) x 2 CPIs at grids 8, 9 and the natural one:
    the static walk's bits, and the first and the last CPI against the fp64 oracle by the gates of tests/gates.py."""
    amb = engine(b2, CFG2, 2, "ticket", 0)
    assert (amb.dims.fft_len, amb.dims.seg_len, amb.dims.n_seg, amb.get_n_delay_bins()) == (1024, 576, 7, 411)
    amb.close()
    o, m, maps, mets = walks_agree(b2, CFG2, "FMT_C32", 2, (8, 9))
    xs, ys = inputs(CFG2, 2)
    d = O.ambiguity_dims(*CFG2, True)
    for c in (0, 1):
        ref = O.ambiguity_process(d, xs[c], ys[c])
        noise, mx = O.map_metrics(ref)
        cell = map_cell_gate(maps[c], ref, peak_tol=PEAK_TOL)
        db = db_map_gate(maps[c], mets[c][0], ref)
        print(f"\n[cfg2 cpi {c}] {cell}\n{db}\nmetrics {mets[c]} against {(noise, mx)}")
        assert cell["ok"], cell
        assert db["ok"], db
        assert abs(mets[c][0] - noise) <= DB_TOL and abs(mets[c][1] - mx) <= DB_TOL
