"""GPU: a bearing per detection -- blah2hip_amb_bearing_dev (bearing_kernel): the snapshot under every record of a detection
list scanned over a steering table on the device, whitened by the CPI's array covariance (the adaptive matched filter) or
not (Bartlett).

No reference counterpart; the oracle is blah2_amd.bearing, the estimator restated in fp64 NumPy with the kernel's explicit
Cholesky and substitution order.  As in tests/test_adaptive_beam_gpu.py the kernel reads any buffer with the map layout, so
the cases upload crafted maps, lists and covariances and the handle is only there for its dimensions (21 x 111).  Every
output is pre-filled with a sentinel and has guard words behind it.

Bounds, per detection, from the oracle's own numbers (nothing is taken from the device's results):
  eps       = 64 K 2^-53 cond(R_l): the relative error of a vector that comes out of the Cholesky solve, the figure the
              weights' test uses for the same factorisation (cond = 1 in Bartlett mode).  The inputs keep cond(R_l) <= 1e5.
  delta     = 6 eps t^H t bounds the error of ANY P(g) = |v^H t|^2 / v^H v: v and t are off by eps each in norm, so v^H t
              by 2 eps |v| |t|, its square over v^H v by 4 eps |t| sqrt(P) + 2 eps P <= 6 eps t^H t since P <= t^H t.
  power     : delta.
  coherence : 8 eps -- delta / t^H t, and t^H t itself is off by 2 eps (coherence <= 1).
  offset    : num = (P- - P+) / 2 is off by delta and den = P- - 2 P0 + P+ by 4 delta, so the quotient by
              (delta + 4 |offset| delta) / (|den| - 4 delta); the test asserts |den| > 8 delta, else the bound says nothing.
  index     : equal wherever the oracle's two largest P differ by 1e-9 of the peak or more (delta / P is 1e-8 at the
              most for cond = 1e5 and coherence near 1, and orders less for the inputs here); no detection may fall under
              that rule -- the excluded count is asserted to be 0.
Largest fractions of the bounds observed on an MI355X over the parity cases and the whole-map lists: power 1.04e-2,
coherence 7.8e-3, offset 4.4e-3.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_crafted as A
import bearing_crafted as B

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 24
SMALL = (-10, 100, -100, 100, 1_000_000, 100_000)    # 21 x 111
EPS64 = 2.0 ** -53
WORST = {"power": 0.0, "coherence": 0.0, "offset": 0.0}


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def amb(b2):
    h = b2.Ambiguity(*SMALL, True, max_batch=MAX_BATCH)
    assert (h.get_n_doppler_bins(), h.get_n_delay_bins()) == (A.ND, A.NC)
    return h


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def guarded_records(torch, b2, n_lists, cap):
    """[n_lists][cap] records, every word the sentinel, and PAD guard words behind them."""
    words = n_lists * cap * b2.BEARING_DTYPE.itemsize // 4
    return torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")


def records(b2, whole, n_lists, cap):
    raw = whole.cpu().numpy().view(np.uint32)
    assert (raw[-PAD:] == GUARD).all()
    return raw[:-PAD].view(b2.BEARING_DTYPE).reshape(n_lists, cap)


def unwritten(rec):
    return (np.ascontiguousarray(rec).view(np.uint32).reshape(rec.shape + (8,)) == GUARD).all(axis=-1)


def make_lists(b2, cells_per_list, cap):
    """Detection lists [n_lists, cap] from (row, col) lists; the slots behind a list's cells hold a record far outside the map
    (read only if the count is wrong)."""
    dets = np.zeros((len(cells_per_list), cap), dtype=b2.DET_DTYPE)
    dets["row"], dets["col"] = 1 << 30, 1 << 30
    for l, cells in enumerate(cells_per_list):
        for i, (r, q) in enumerate(cells):
            dets[l, i]["row"], dets[l, i]["col"] = r, q
            dets[l, i]["snr"] = 10.0 + i
    return dets


def upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32, R=None, loading=0.0, wrap=False):
    """One call on uploaded lists -> the records [n_lists, cap] (sentinel where nothing was written)."""
    n_lists, cap = dets.shape
    d_dets, d_cnt, d_steer = upload(torch, dets), upload(torch, np.asarray(counts, dtype=np.uint32)), upload(torch, steer32)
    d_cov = upload(torch, np.asarray(R, dtype=np.complex128)) if R is not None else None
    whole = guarded_records(torch, b2, n_lists, cap)
    amb.bearing_dev(d_maps.data_ptr(), K, n_cpi, d_dets.data_ptr(), cap, d_cnt.data_ptr(), n_lists, d_steer.data_ptr(),
                    steer32.shape[0], whole.data_ptr(), d_cov.data_ptr() if d_cov is not None else None, loading, wrap,
                    stream(torch))
    torch.cuda.synchronize()
    return records(b2, whole, n_lists, cap)


def check_list(b2, rec, snap, steer32, R, loading, wrap, tag):
    """The records of one list against blah2_amd.bearing on the same snapshots, within the bounds of the module docstring."""
    K, G = snap.shape[1], steer32.shape[0]
    P, tt, usable, _ = b2.process.bearing_powers(snap, steer32, R, loading)
    idx, off, power, coh, adaptive = b2.bearing(snap, steer32, R, loading, wrap)
    assert usable.all(), tag
    cond = 1.0 if R is None else np.linalg.cond(R + loading * (np.trace(R).real / K) * np.eye(K))
    assert cond <= 1e5, (tag, cond)
    eps = 64 * K * EPS64 * cond
    delta = 6 * eps * tt
    excluded = int((B.top_two_gap(snap, steer32, R, loading) < 1e-9).sum())
    assert excluded == 0, (tag, excluded)
    assert np.array_equal(rec["index"], idx), (tag, rec["index"], idx)
    assert np.array_equal(rec["adaptive"], adaptive), tag
    rows = np.arange(len(idx))
    pm, p0, pp = P[rows, (idx - 1) % G], P[rows, idx], P[rows, (idx + 1) % G]
    den = np.abs((pm - 2.0 * p0) + pp)
    refined = ((idx > 0) & (idx < G - 1)) | wrap
    assert (den[refined] > 8 * delta[refined]).all(), tag
    off_bound = np.where(refined, (delta + 4 * np.abs(off) * delta) / np.where(refined, den - 4 * delta, 1.0), 0.0)
    assert (rec["offset"][~refined] == 0).all(), tag
    frac = {"power": np.abs(rec["power"] - power) / delta, "coherence": np.abs(rec["coherence"] - coh) / (8 * eps),
            "offset": (np.abs(rec["offset"] - off)[refined] / off_bound[refined]) if refined.any() else np.zeros(1)}
    for name, f in frac.items():
        WORST[name] = max(WORST[name], float(f.max()))
        assert (f <= 1.0).all(), (tag, name, float(f.max()))
    assert ((rec["coherence"] >= 0) & (rec["coherence"] <= 1 + 8 * eps)).all(), tag
    return {k: float(v.max()) for k, v in frac.items()}


def random_cells(rng, n):
    return [(int(r), int(q)) for r, q in zip(rng.integers(0, A.ND, n), rng.integers(0, A.NC, n))]


# ---- 1. parity with blah2_amd.bearing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [3, 64, 65, 177, 384])
@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_parity_with_the_numpy_estimator(b2, torch, amb, K, G):
    """Both modes, one and three CPIs, n_lists = n_cpi and 2 n_cpi (list l reads the maps AND the covariance of CPI
    l mod n_cpi: the CPIs differ, so a wrong one shows), lists of 24 slots (two chunks of 16, counts that end inside either)
    on random noise cells plus the scene's three cells."""
    cap = 24
    steer32 = B.ula_table(K, np.linspace(-88.0, 88.0, G))
    worst = {"power": 0.0, "coherence": 0.0, "offset": 0.0}
    for n_cpi in (1, 3):
        maps = B.scene_k(K, n_cpi, seed=5000 + 100 * K + n_cpi)
        d_maps = torch.from_numpy(maps).cuda()
        Rs = A.covariance64(maps)
        for mult in (1, 2):
            n_lists = mult * n_cpi
            rng = np.random.default_rng(5300 + 10 * K + G + n_lists)
            counts = [(24, 19, 7, 16, 17, 1)[l] for l in range(n_lists)]
            cells = [(list(B.CELLS) + random_cells(rng, cap))[:counts[l]] for l in range(n_lists)]
            dets = make_lists(b2, cells, cap)
            for R, loading in ((None, 0.0), (Rs, B.LOADING)):
                rec = run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32, R, loading)
                for l in range(n_lists):
                    c = l % n_cpi
                    assert unwritten(rec[l, counts[l]:]).all() and not unwritten(rec[l, :counts[l]]).any()
                    f = check_list(b2, rec[l, :counts[l]], B.snapshots(maps, c, cells[l]), steer32,
                                   None if R is None else R[c], loading, False,
                                   f"K={K} G={G} n_cpi={n_cpi} n_lists={n_lists} list {l} {'adaptive' if R is not None else 'Bartlett'}")
                    worst = {k: max(worst[k], f[k]) for k in f}
    print(f"bearing K={K} G={G}: largest error / bound: power {worst['power']:.3e}, coherence {worst['coherence']:.3e}, "
          f"offset {worst['offset']:.3e} (all cases so far: {WORST})")


def test_every_cell_of_the_map_in_strided_chunks(b2, torch, amb):
    """Lists that hold every cell of the map, 24 of them: more chunks than workgroups, so a workgroup walks several."""
    K, n_cpi, n_lists, G = 2, 3, 24, 65
    cap = A.ND * A.NC
    maps = B.scene_k(K, n_cpi, seed=5900)
    Rs = A.covariance64(maps)
    steer32 = B.ula_table(K, np.linspace(-88.0, 88.0, G))
    every = [(r, q) for r in range(A.ND) for q in range(A.NC)]
    counts = [cap - 5 * l for l in range(n_lists)]
    dets = make_lists(b2, [every[5 * l:] for l in range(n_lists)], cap)
    rec = run(torch, b2, amb, torch.from_numpy(maps).cuda(), K, n_cpi, dets, counts, steer32, Rs, B.LOADING)
    from blah2_amd import _lib
    X = amb.info(_lib.INFO_BEARING_GRID)
    assert 1 <= X < (cap + 15) // 16
    for l in range(n_lists):
        assert unwritten(rec[l, counts[l]:]).all()
        check_list(b2, rec[l, :counts[l]], B.snapshots(maps, l % n_cpi, every[5 * l:]), steer32, Rs[l % n_cpi], B.LOADING, False,
                   f"every cell, list {l}")
    print(f"every cell: {X} workgroups per list for {(cap + 15) // 16} chunks; largest error / bound so far {WORST}")


# ---- 2. the scene: covariance, detections, bearing -----------------------------------------------------------------------
def test_the_scene_on_the_device(b2, torch, amb):
    """The shared cell reads the interferer in Bartlett mode and the target in adaptive mode, with the covariance
    blah2hip_amb_covariance_dev leaves on the device."""
    K = B.K
    maps = B.scene()
    d_maps = torch.from_numpy(maps).cuda()
    d_cov = torch.zeros((1, K, K), dtype=torch.complex128, device="cuda")
    cells = list(B.CELLS) + random_cells(np.random.default_rng(6000), 29)
    cap = len(cells)
    dets = make_lists(b2, [cells], cap)
    steer32 = B.ula_table()
    d_dets, d_cnt, d_steer = upload(torch, dets), upload(torch, np.array([cap], dtype=np.uint32)), upload(torch, steer32)
    st = stream(torch)
    whole_b, whole_a = guarded_records(torch, b2, 1, cap), guarded_records(torch, b2, 1, cap)
    amb.covariance_dev(d_maps.data_ptr(), K, 1, d_cov.data_ptr(), None, st)
    amb.bearing_dev(d_maps.data_ptr(), K, 1, d_dets.data_ptr(), cap, d_cnt.data_ptr(), 1, d_steer.data_ptr(), len(steer32),
                    whole_b.data_ptr(), stream=st)
    amb.bearing_dev(d_maps.data_ptr(), K, 1, d_dets.data_ptr(), cap, d_cnt.data_ptr(), 1, d_steer.data_ptr(), len(steer32),
                    whole_a.data_ptr(), d_cov.data_ptr(), B.LOADING, False, st)
    torch.cuda.synchronize()
    bart, adap = records(b2, whole_b, 1, cap)[0], records(b2, whole_a, 1, cap)[0]
    R = d_cov.cpu().numpy()[0]
    snap = B.snapshots(maps, 0, cells)
    check_list(b2, bart, snap, steer32, None, 0.0, False, "the scene, Bartlett")
    check_list(b2, adap, snap, steer32, R, B.LOADING, False, "the scene, adaptive")
    deg_b = b2.bearing_degrees(bart["index"], bart["offset"], B.ULA_DEG)
    deg_a = b2.bearing_degrees(adap["index"], adap["offset"], B.ULA_DEG)
    print(f"shared cell: Bartlett {deg_b[0]:+.3f} deg, adaptive {deg_a[0]:+.3f} deg; target cell: Bartlett {deg_b[1]:+.3f} deg, "
          f"adaptive {deg_a[1]:+.3f} deg; interferer cell: Bartlett {deg_b[2]:+.3f} deg")
    assert abs(deg_b[0] - A.INTERFERER_DEG) <= 0.5 and abs(deg_a[0] - A.TARGET_DEG) <= 0.5
    assert abs(deg_b[1] - A.TARGET_DEG) <= 0.5 and abs(deg_a[1] - A.TARGET_DEG) <= 0.5
    assert abs(deg_b[2] - A.INTERFERER_DEG) <= 0.5


# ---- 3. / 4. the identity and covariances that cannot be factorised --------------------------------------------------------
def same_bits_but_adaptive(x, y):
    return all(x[f].tobytes() == y[f].tobytes() for f in ("index", "offset", "power", "coherence"))


@pytest.mark.parametrize("K", [2, 4, 8])
def test_an_identity_covariance_gives_the_bartlett_bits(b2, torch, amb, K):
    n_cpi, cap = 2, 20
    maps = B.scene_k(K, n_cpi, seed=7000 + K)
    d_maps = torch.from_numpy(maps).cuda()
    rng = np.random.default_rng(7100 + K)
    cells = [list(B.CELLS) + random_cells(rng, cap - 3) for _ in range(n_cpi)]
    dets = make_lists(b2, cells, cap)
    steer32 = B.ula_table(K)
    eye = np.broadcast_to(np.eye(K, dtype=np.complex128), (n_cpi, K, K)).copy()
    bart = run(torch, b2, amb, d_maps, K, n_cpi, dets, [cap, cap], steer32)
    iden = run(torch, b2, amb, d_maps, K, n_cpi, dets, [cap, cap], steer32, eye, 0.0)
    assert (bart["adaptive"] == 0).all() and (iden["adaptive"] == 1).all() and (bart["index"] >= 0).all()
    assert same_bits_but_adaptive(bart, iden)


def test_failed_factorisations_fall_back_and_leave_their_neighbours_alone(b2, torch, amb):
    K, n_cpi, cap = 4, 3, 20
    maps = B.scene_k(K, n_cpi, seed=7200)
    d_maps = torch.from_numpy(maps).cuda()
    rng = np.random.default_rng(7201)
    cells = [list(B.CELLS) + random_cells(rng, cap - 3) for _ in range(n_cpi)]
    dets = make_lists(b2, cells, cap)
    counts = [cap] * n_cpi
    steer32 = B.ula_table(K)
    Rs = A.covariance64(maps)
    Rs[1] = 0
    Rs[2, 3, 1] = complex(np.nan, 0.0)  # in the lower triangle
    rec = run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32, Rs, B.LOADING)
    bart = run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32)
    assert (rec["adaptive"][0] == 1).all() and (rec["adaptive"][1:] == 0).all() and (rec["index"] >= 0).all()
    for c in (1, 2):
        assert np.array_equal(rec[c].view(np.uint32), bart[c].view(np.uint32)), c
    assert not same_bits_but_adaptive(rec[0], bart[0])
    # the healthy CPI alone: the same bits
    alone = run(torch, b2, amb, torch.from_numpy(np.ascontiguousarray(maps[:, :1])).cuda(), K, 1, dets[:1], counts[:1], steer32,
                Rs[:1], B.LOADING)
    assert np.array_equal(alone[0].view(np.uint32), rec[0].view(np.uint32))
    check_list(b2, rec[0], B.snapshots(maps, 0, cells[0]), steer32, Rs[0], B.LOADING, False, "the healthy CPI")


# ---- 5. what is written -----------------------------------------------------------------------------------------------------
def test_what_is_written(b2, torch, amb):
    K, n_cpi, cap = 4, 1, 20
    maps = B.scene_k(K, n_cpi, seed=7300)
    maps[:, 0, 2, 5] = 0                     # a zero snapshot
    maps[1, 0, 3, 6] = np.nan                # one NaN among finite cells
    maps[:, 0, 3, 7] = np.inf
    maps[3, 0, 3, 8] = complex(0.0, -np.inf)
    maps[0, 0, 3, 9] = 0                     # one zero among nonzero cells: an ordinary snapshot
    d_maps = torch.from_numpy(maps).cuda()
    outside = [(-1, 5), (A.ND, 5), (4, -1), (4, A.NC), (-(1 << 31), 0), ((1 << 31) - 1, (1 << 31) - 1)]
    cells = [(2, 5), (3, 6), (3, 7), (3, 8), (3, 9)] + outside + list(B.CELLS) + random_cells(np.random.default_rng(7301), 6)
    assert len(cells) == cap
    steer32 = B.ula_table(K)
    R = A.covariance64(B.scene_k(K, n_cpi, seed=7300))
    n_lists = 4  # counts 0, under cap, cap and beyond cap
    dets = make_lists(b2, [cells] * n_lists, cap)
    counts = [0, 13, cap, cap + 1000]
    for Rm, loading in ((None, 0.0), (R, B.LOADING)):
        rec = run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32, Rm, loading)
        for l, n in enumerate(min(c, cap) for c in counts):
            un = unwritten(rec[l])
            want = np.array([i >= n or 5 <= i < 5 + len(outside) for i in range(cap)])
            assert np.array_equal(un, want), (l, un)
            for i in range(min(n, 4)):  # zero, NaN, inf, -inf: no estimate, every other field 0
                assert rec[l, i].tolist() == (-1, 0, 0.0, 0.0, 0.0), (l, i, rec[l, i])
            if n > 4:
                assert rec[l, 4]["index"] >= 0
            live = [i for i in range(n) if i >= 4 and not want[i]]
            if live:
                check_list(b2, rec[l, live], B.snapshots(maps, 0, [cells[i] for i in live]), steer32,
                           None if Rm is None else Rm[0], loading, False, f"what is written, list {l}")


# ---- 6. the closed grid -------------------------------------------------------------------------------------------------
def test_wrap_refines_across_the_seam(b2, torch, amb):
    """Noise-free plane waves on a four-element circle, scanned on a 360-point grid: 0.4 and 359.6 degrees peak at index 0 from
    either side of the seam, 359.4 at index 359."""
    K = 4
    sources = (0.4, 359.6, 359.4, 180.3)
    maps = np.zeros((K, 1, A.ND, A.NC), dtype=np.complex64)
    cells = [(3, 10 + i) for i in range(len(sources))]
    for (r, q), deg in zip(cells, sources):
        maps[:, 0, r, q] = ((2.0 - 1.0j) * b2.uca_steering(K, B.UCA_RADIUS, [deg])[0]).astype(np.complex64)
    d_maps = torch.from_numpy(maps).cuda()
    steer32 = B.uca_table(K)
    dets = make_lists(b2, [cells], len(cells))
    snap = B.snapshots(maps, 0, cells)
    for wrap in (False, True):
        rec = run(torch, b2, amb, d_maps, K, 1, dets, [len(cells)], steer32, wrap=wrap)[0]
        check_list(b2, rec, snap, steer32, None, 0.0, wrap, f"UCA wrap={wrap}")
        assert rec["index"].tolist() == [0, 0, 359, 180]
        deg = b2.bearing_degrees(rec["index"], rec["offset"], B.UCA_DEG, wrap=True)
        if wrap:
            assert (rec["offset"][:3] != 0).all() and rec["offset"][0] > 0 > rec["offset"][1] and rec["offset"][2] > 0
            assert (np.abs((deg - np.array(sources) + 180.0) % 360.0 - 180.0) <= 0.05).all(), deg
        else:
            assert (rec["offset"][:3] == 0).all() and abs(deg[3] - 180.3) <= 0.05


# ---- 7. the same bits twice, and from a graph -------------------------------------------------------------------------------
def test_the_same_bits_twice_and_from_a_graph(b2, torch, amb):
    K, n_cpi, cap, n_lists = 8, 3, 40, 6
    maps = B.scene_k(K, n_cpi, seed=7500)
    d_maps = torch.from_numpy(maps).cuda()
    rng = np.random.default_rng(7501)
    dets = make_lists(b2, [random_cells(rng, cap) for _ in range(n_lists)], cap)
    counts = [40, 33, 1, 16, 17, 39]
    steer32 = B.ula_table(K, np.linspace(-88.0, 88.0, 384))
    Rs = A.covariance64(maps)
    first = run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32, Rs, B.LOADING)
    second = run(torch, b2, amb, d_maps, K, n_cpi, dets, counts, steer32, Rs, B.LOADING)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))

    d_dets, d_cnt, d_steer = upload(torch, dets), upload(torch, np.asarray(counts, dtype=np.uint32)), upload(torch, steer32)
    d_cov = upload(torch, Rs)
    whole = guarded_records(torch, b2, n_lists, cap)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one stream, one kernel node: no parallel branches
        amb.bearing_dev(d_maps.data_ptr(), K, n_cpi, d_dets.data_ptr(), cap, d_cnt.data_ptr(), n_lists, d_steer.data_ptr(),
                        len(steer32), whole.data_ptr(), d_cov.data_ptr(), B.LOADING, False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert unwritten(records(b2, whole, n_lists, cap)).all()  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(records(b2, whole, n_lists, cap).view(np.uint32), first.view(np.uint32))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(b2, torch, amb):
    from blah2_amd import _lib
    L, h = amb._L, amb._h
    K, n_cpi, cap, n_lists = 4, 3, 16, 6
    d_maps = torch.from_numpy(B.scene_k(8, n_cpi, seed=7600)).cuda()
    dets = make_lists(b2, [list(B.CELLS)] * n_lists, cap)
    d_dets, d_cnt = upload(torch, dets), upload(torch, np.full(n_lists, 3, dtype=np.uint32))
    d_steer = upload(torch, B.ula_table(8, np.linspace(-88.0, 88.0, 385)))
    d_cov = upload(torch, np.broadcast_to(np.eye(8, dtype=np.complex128), (n_cpi, 8, 8)).copy())
    whole = guarded_records(torch, b2, n_lists, cap)
    # (d_map, n_surv, n_cpi, d_dets, cap, d_count, n_lists, d_cov, loading, d_steer, n_grid, flags, d_out)
    good = [d_maps.data_ptr(), K, n_cpi, d_dets.data_ptr(), cap, d_cnt.data_ptr(), n_lists, d_cov.data_ptr(), 1e-3,
            d_steer.data_ptr(), 177, 0, whole.data_ptr()]
    bad = {
        "NULL list": {3: None}, "NULL count": {5: None}, "NULL steering table": {9: None}, "NULL output": {12: None},
        "cap 0": {4: 0}, "n_cpi 0": {2: 0}, "n_lists 0": {6: 0}, "n_lists not a multiple of n_cpi": {6: 4},
        "n_lists below n_cpi": {6: 2}, "n_surv 0": {1: 0}, "n_surv 1": {1: 1}, "n_surv 9": {1: 9, 2: 1, 6: 1},
        "n_surv * n_cpi above max_batch": {1: 8, 2: 4, 6: 4}, "n_grid 0": {10: 0}, "n_grid 2": {10: 2}, "n_grid 385": {10: 385},
        "flag bit 1": {11: 2}, "flag bit 31": {11: 0x80000001}, "loading < 0": {8: -1e-3}, "loading nan": {8: float("nan")},
        "loading inf": {8: float("inf")},
    }
    for name, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_bearing_dev(h, *args, None) == _lib.ERR_INVALID, name
    assert L.blah2hip_amb_bearing_dev(None, *good, None) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == GUARD).all()
    # the loading is not looked at without a covariance; the largest grid and the wrap flag are accepted
    for change in ({7: None, 8: float("nan")}, {7: None, 8: -1.0}, {10: 384}, {10: 3}, {11: _lib.BEARING_WRAP}, {1: 2}, {1: 8}):
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert L.blah2hip_amb_bearing_dev(h, *args, None) == _lib.OK, change
    torch.cuda.synchronize()
    rec = records(b2, whole, n_lists, cap)
    assert not unwritten(rec[:, :3]).any() and unwritten(rec[:, 3:]).all()


# ---- 9. the timing slot -----------------------------------------------------------------------------------------------------
def test_the_timing_slot_counts_one_launch(b2, torch, amb):
    from blah2_amd import _lib
    K = 4
    d_maps = torch.from_numpy(B.scene()).cuda()
    dets = make_lists(b2, [list(B.CELLS)], 3)
    amb.set_timing(True)
    try:
        amb.get_timing()  # clears whatever earlier calls left
        rec = run(torch, b2, amb, d_maps, K, 1, dets, [3], B.ula_table())
        t = amb.get_timing()
    finally:
        amb.set_timing(False)
    assert (rec["index"] >= 0).all()
    assert t["bearing"][1] == 1 and t["bearing"][0] > 0.0
    assert all(n == 0 for name, (ms, n) in t.items() if name != "bearing")
    assert _lib.KERNEL_NAMES[_lib.K_BEARING] == "bearing" and _lib.K_COUNT == 10
    assert amb.info(_lib.INFO_BEARING_GRID) == 1
