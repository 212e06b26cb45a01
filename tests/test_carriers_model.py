"""CPU: the multi-carrier integration's definition, pinned on its fp64 restatement (``blah2_amd.carrier_table``,
``blah2_amd.fuse_carriers``), the fp32 emulation of the kernel's arithmetic against the derived bound, and the replay plan.

The library's own table (``blah2hip_carrier_table``) reads the Doppler axis of an ambiguity handle, which needs a device:
tests/test_carriers_gpu.py compares it with the restatement entry by entry.  Here the restatement is compared with a
brute-force evaluation of the header's definition, one Python float at a time.

``test_the_aligned_sum_finds_the_echo``: on ``carrier_scenes.noise_scene`` (seed fixed) the echo's cell of the aligned sum is
the map's strongest, 3.42 (power 11.7 over a map mean of 1.0), and stands above the strongest cell of the sum taken row by
row, 2.18 (power 4.75), by a factor of 1.57 in amplitude, 3.9 dB in power; the echo's own cell of that unaligned sum holds
2.07.  (fp64, this seed; over many draws the powers average 9.2 and 4.5.)  The assertion is the ordering.
"""
import math

import numpy as np
import pytest

import carrier_scenes as S
import integrate_crafted as IC
from blah2_amd import _lib, carrier_ratios, carrier_table, fuse_carriers, integrate_maps
from blah2_amd.chain_plan import plan_chain

AXES = {
    "21": (np.arange(21) - 10) * 1.0,
    "48": (np.arange(48) - 24) * 0.5,
    "513": (np.arange(513) - 256) * 2.0,
    "21-asymmetric": (np.arange(21) - 4) * 1.5,  # -6 .. 24
    "21-positive": 6.0 + np.arange(21) * 1.5,    # 6 .. 36: ratio 0.5 leaves it at the bottom, ratio 2 at the top
    "2": np.array([-1.0, 1.0]),
}
RATIO_SETS = {
    "ones": (1.0, 1.0, 1.0),
    "physical": (1.0, 1.004, 0.996, 1.02),
    "exaggerated": (1.0, 1.25, 0.8, 1.1),
    "clamped": (1.0, 2.0, 0.5),
}


def brute(axis, ratio, interp):
    """The header's definition, one float at a time."""
    nD = len(axis)
    d0, delta = float(axis[0]), (float(axis[nD - 1]) - float(axis[0])) / (nD - 1)
    row, a_lo, a_hi, covered = [], [], [], [0] * nD
    for r in ratio:
        rr, lo, hi = [], [], []
        for j in range(nD):
            u = (float(r) * float(axis[j]) - d0) / delta
            if abs(u - round(u)) <= 1e-9:
                u = float(round(u))
            if 0.0 <= u <= nD - 1:
                covered[j] += 1
            u = min(max(u, 0.0), float(nD - 1))
            if interp == "nearest":
                rr.append(math.floor(u + 0.5)), lo.append(np.float32(1)), hi.append(np.float32(0))
            else:
                k = math.floor(u)
                rr.append(k), lo.append(np.float32(1.0 - (u - k))), hi.append(np.float32(u - k))
        row.append(rr), a_lo.append(lo), a_hi.append(hi)
    return np.array(row), np.array(a_lo, dtype=np.float32), np.array(a_hi, dtype=np.float32), np.array(covered)


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("axis", ["21", "48", "513", "21-asymmetric", "21-positive", "2"])
def test_ratio_one_is_the_identity(axis, interp):
    a = AXES[axis]
    t = carrier_table(a, [1.0, 1.0], interp)
    assert np.array_equal(t["row"], np.tile(np.arange(a.size), (2, 1)))
    assert np.all(t["a_lo"] == 1) and np.all(t["a_hi"] == 0) and np.all(t["covered"] == 2)
    assert t["row"].dtype == np.int32 and t["a_lo"].dtype == np.float32 and t["covered"].dtype == np.uint32


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("ratios", list(RATIO_SETS))
@pytest.mark.parametrize("axis", list(AXES))
def test_table_against_the_definition(axis, ratios, interp):
    a, r = AXES[axis], RATIO_SETS[ratios]
    t = carrier_table(a, r, interp)
    row, a_lo, a_hi, covered = brute(a, r, interp)
    assert np.array_equal(t["row"], row) and np.array_equal(t["covered"], covered)
    assert np.array_equal(t["a_lo"], a_lo) and np.array_equal(t["a_hi"], a_hi)
    assert np.all(np.diff(t["row"], axis=1) >= 0)  # rows never descend along the axis
    assert t["row"].min() >= 0 and t["row"].max() <= a.size - 1
    assert np.all(t["a_hi"][t["row"] == a.size - 1] == 0)  # row + 1 is never read off the map
    assert np.array_equal(t["covered"], len(r) - S.uncovered(a, r).sum(axis=0))  # a direct count


@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_clamping_at_both_ends(interp):
    a = AXES["21-positive"]
    t = carrier_table(a, [1.0, 2.0, 0.5], interp)
    out = S.uncovered(a, [1.0, 2.0, 0.5])
    assert out[1].any() and out[2].any() and not out[0].any()
    assert np.all(t["row"][1][out[1]] == a.size - 1) and np.all(t["row"][2][out[2]] == 0)  # the edge row stands in
    assert np.all(t["a_lo"][out] == 1) and np.all(t["a_hi"][out] == 0)
    assert np.array_equal(t["covered"], 3 - out.sum(axis=0)) and t["covered"].min() == 2
    # a symmetric axis under ratio 2: both ends in one carrier
    t = carrier_table(AXES["21"], [1.0, 2.0], interp)
    assert np.array_equal(t["row"][1], np.clip(2 * np.arange(21) - 10, 0, 20))
    assert np.array_equal(t["covered"], np.where(np.abs(np.arange(21) - 10) <= 5, 2, 1))


def test_refusals_of_the_table():
    a = AXES["21"]
    for bad in ([], [1.0] * 9, [float("nan")], [float("inf")], [0.49], [2.01], [1.0, -1.0]):
        with pytest.raises(ValueError):
            carrier_table(a, bad, "nearest")
    for interp in ("cubic", 2, -1, None, True):
        with pytest.raises(ValueError):
            carrier_table(a, [1.0], interp)
    with pytest.raises(ValueError):
        carrier_table([0.0], [1.0], "nearest")
    assert np.array_equal(carrier_table(a, [1.0], _lib.CARRIER_LINEAR)["row"], carrier_table(a, [1.0], "linear")["row"])
    assert np.allclose(carrier_ratios(100.0, [5.0, -5.0, 0.0]), [1.0, 95.0 / 105.0, 100.0 / 105.0])
    with pytest.raises(ValueError):
        carrier_ratios(100.0, [0.0, -100.0])


def test_the_library_refuses_without_a_handle(built_lib):
    """What the host-only entry points can be asked without a device: a NULL handle."""
    r = (_lib.C.c_double * 1)(1.0)
    assert built_lib.blah2hip_carrier_table(None, r, 1, 0, None, None, None, None) == _lib.ERR_INVALID
    assert built_lib.blah2hip_amb_set_carriers(None, r, 1, 0) == _lib.ERR_INVALID
    assert built_lib.blah2hip_amb_fuse_carriers_dev(None, None, 1, None, None, None, None) == _lib.ERR_INVALID
    assert (_lib.MAX_CARRIERS, _lib.CARRIER_NEAREST, _lib.CARRIER_LINEAR, _lib.INFO_CARRIER_GRID) == (8, 0, 1, 22)
    assert _lib.MAX_CARRIERS >= _lib.MAX_DDC_CARRIERS


@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_all_ratios_one_is_the_integrator(interp):
    m = IC.maps(3, 2, 21, 37, seed=5)
    w = (1.0, 0.25, 4.0)
    t = carrier_table(AXES["21"], [1.0] * 3, interp)
    assert np.array_equal(fuse_carriers(m, t, w), integrate_maps(m, w, window=1))
    assert np.array_equal(fuse_carriers(m, t), integrate_maps(m, window=1))


def test_a_nan_reaches_the_cells_that_read_it_and_no_other():
    m = IC.maps(2, 1, 21, 8, seed=6).astype(np.complex128)
    m[1, 0, 20, 3] = np.nan  # carrier 1's top row
    for interp in ("nearest", "linear"):
        t = carrier_table(AXES["21"], [1.0, 0.8], interp)
        out = fuse_carriers(m, t)
        reads = (t["row"][1] == 20) | ((t["row"][1] == 19) & (t["a_hi"][1] != 0))
        want = np.zeros((1, 21, 8), dtype=bool)
        want[0, reads, 3] = True
        assert np.array_equal(np.isnan(out), want)


def test_the_aligned_sum_finds_the_echo():
    m, (row, col) = S.noise_scene()
    axis = S.scene_axis()
    aligned = fuse_carriers(m, carrier_table(axis, S.RATIOS, "nearest"))[0]
    unaligned = fuse_carriers(m, carrier_table(axis, [1.0] * len(S.RATIOS), "nearest"))[0]
    print(f"aligned echo {aligned[row, col]:.3f} (power {aligned[row, col] ** 2:.2f}), map mean power {np.mean(aligned ** 2):.3f}; "
          f"unaligned strongest {unaligned.max():.3f} (power {unaligned.max() ** 2:.2f}), its echo cell {unaligned[row, col]:.3f}")
    assert np.unravel_index(np.argmax(aligned), aligned.shape) == (row, col)
    assert aligned[row, col] > unaligned.max() > unaligned[row, col]


CASES = [("exaggerated", "nearest", None), ("exaggerated", "linear", (1.0, 0.25, 4.0, 2.0)), ("clamped", "linear", (1.0, 0.25, 4.0)),
         ("physical", "linear", None), ("ones", "nearest", (1.0, 0.25, 4.0))]


@pytest.mark.parametrize("ratios,interp,w", CASES)
def test_the_emulation_stays_inside_the_bound(ratios, interp, w):
    r = RATIO_SETS[ratios]
    m = IC.maps(len(r), 2, 21, 37, seed=7)
    t = carrier_table(AXES["21"], r, interp)
    ref = fuse_carriers(m, t, w)
    err = np.abs(S.emulate(m, t, w).astype(np.float64) - ref)
    worst = float(np.max(err / S.bound(len(r), ref)))
    print(f"{ratios} {interp}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_mutant_misses_the_bound_tenfold(mutant):
    r = RATIO_SETS["clamped"] if mutant == "clamped-zero" else RATIO_SETS["exaggerated"]
    w = (1.0, 0.25, 4.0, 2.0)[:len(r)]
    m = IC.maps(len(r), 2, 21, 37, seed=8)
    t = carrier_table(AXES["21"], r, "linear")
    ref = fuse_carriers(m, t, w)
    out = S.emulate(m, t, w, mutant=mutant, out_of_axis=S.uncovered(AXES["21"], r))
    worst = float(np.max(np.abs(out.astype(np.float64) - ref) / S.bound(len(r), ref)))
    print(f"{mutant}: largest error / bound {worst:.3g}")
    assert worst >= 10.0


# ---- the replay plan ------------------------------------------------------------------------------------------------------
FS = N = 65536
FC = 655360.0
DET = dict(enable=True, pfa=1e-5, nGuard=2, nTrain=6, minDelay=0, minDoppler=5.0, nCentroid=3)


def config(offset, fc=FC, amb=None, det=None, ddc=None, **extra):
    cfg = dict({"fs": FS, "n_samples": N,
                "ambiguity": dict({"delayMin": -4, "delayMax": 20, "dopplerMin": -64, "dopplerMax": 64}, **(amb or {})),
                "detection": dict(DET, **(det or {})), "clutter": {"enable": False},
                "ddc": dict({"offset": offset, "decimation": 4, "taps": 64}, **(ddc or {}))}, **extra)
    if fc is not None:
        cfg["fc"] = fc
    return cfg


def same_plan(p, q):
    for k in p.__dataclass_fields__:
        a, b = getattr(p, k), getattr(q, k)
        if k == "ddc":
            assert set(a) == set(b) and all(np.array_equal(a[i], b[i]) for i in a), k
        else:
            assert a == b, k


def test_a_list_of_one_offset_plans_as_the_scalar():
    same_plan(plan_chain(config([16384.0])), plan_chain(config(16384.0)))
    same_plan(plan_chain(config([16384.0], fc=None)), plan_chain(config(16384.0, fc=None)))  # one carrier needs no capture.fc
    p = plan_chain(config(16384.0))
    assert p.carriers is None and p.carrier_interp == "nearest" and p.ddc["offset"] == 16384.0


def test_several_offsets_plan_carriers():
    p = plan_chain(config([-16384.0, 16384.0], ddc={"interp": "linear"}, integrate={"window": 4}))
    assert p.carriers == (-16384.0, 16384.0) and p.carrier_interp == "linear" and p.carrier_fc == FC
    assert p.ddc["offset"] == -16384.0 and p.integrate == (4, 1) and p.needs_order and p.detect == "device"
    assert plan_chain(config((0.0, 1000.0))).carrier_interp == "nearest"


TWO = [-16384.0, 16384.0]
REFUSALS = [
    (dict(offset=TWO, amb={"migration": {"fc": FC}}), "ambiguity.migration"),
    (dict(offset=TWO, amb={"dopplerRate": 2}), "ambiguity.dopplerRate"),
    (dict(offset=TWO, integrate={"window": 2, "tracks": {"fc": FC}}), "integrate.tracks"),
    (dict(offset=TWO, det={"clutterMap": {"memory": 8}}), "detection.clutterMap"),
    (dict(offset=TWO, det={"clean": {"snr": 18}}), "detection.clean"),
    (dict(offset=[float(1000 * i) for i in range(9)]), "9 offsets"),
    (dict(offset=[]), "0 offsets"),
    (dict(offset=[1000.0, 2000.0, 1000.0]), "same offset"),
    (dict(offset=[-16384.0, 16384.0], fc=16384.0), "not a positive"),
    (dict(offset=TWO, fc=None), "capture.fc"),
    (dict(offset=TWO, ddc={"interp": "cubic"}), "interp"),
    (dict(offset=[0.0, 40000.0]), "beyond fs / 2"),
    (dict(offset=TWO, integrate={"window": 600}), "looks"),
]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_the_plan_refuses_naming_capture_ddc(kw, text):
    with pytest.raises(ValueError, match="capture.ddc") as e:
        plan_chain(config(**kw))
    assert text in str(e.value)


def test_the_plan_refuses_host_detection():
    with pytest.raises(ValueError, match="capture.ddc") as e:
        plan_chain(config(TWO), detect="host")
    assert "--detect host" in str(e.value)
    plan_chain(config(TWO[0]), detect="host")  # one carrier: as before
