"""CPU suite for the 8-bit sample format: the Cs8Pair reader (two files of int8 I, Q pairs) against NumPy slicing in
every read mode, the sharded replay with a stub processor, the CLI's arguments, the ABI's two new codes and symbol,
and the index algebra of InI8 / InI8C32 on the host (tests/host/emulate_i8.cpp)."""
import json
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import yaml

from blah2_amd import _lib
from blah2_amd import replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000  # samples per CPI


def write_pair(tmp_path, nx, ny, seed=1, odd_x=False, odd_y=False):
    """Two files of nx / ny int8 pairs (plus a dangling byte when asked); (path_x, path_y, x [nx, 2], y [ny, 2])."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-128, 128, size=(nx, 2), dtype=np.int64).astype(np.int8)
    y = rng.integers(-128, 128, size=(ny, 2), dtype=np.int64).astype(np.int8)
    px, py = str(tmp_path / "ref.cs8"), str(tmp_path / "surv.cs8")
    for p, a, odd in ((px, x, odd_x), (py, y, odd_y)):
        with open(p, "wb") as f:
            f.write(a.tobytes())
            if odd:
                f.write(b"\x55")
    return px, py, x, y


def want_batch(x, y, k0, cnt, n=N, sx=0, sy=0):
    return np.stack([np.stack([x[sx + k * n:sx + (k + 1) * n], y[sy + k * n:sy + (k + 1) * n]]) for k in range(k0, k0 + cnt)])


@pytest.mark.parametrize("how", ["memmove", "pread", "mapped"])
def test_cs8pair_reads_equal_numpy_slicing(tmp_path, how):
    """Files of unequal length with odd byte counts and both skips; whole batches and the ragged last one."""
    px, py, x, y = write_pair(tmp_path, 7 * N + 123, 5 * N + 7 + 400, odd_x=True, odd_y=True)
    f = R.Cs8Pair(px, py, N, skip_x=3, skip_y=7)
    assert f.layout == "cs8" and f.n_cpis == 5  # what BOTH files hold: (5400 + 7 - 7) // 1000
    for k0, cnt in R.shard_batches(f.n_cpis, 2, 0, 1):
        want = want_batch(x, y, k0, cnt, sx=3, sy=7)
        assert np.array_equal(f.batch(range(k0, k0 + cnt)), want)
        off, nbytes, first = f.extent(k0, cnt)
        assert (nbytes, first) == (2 * cnt * N * 2, 0)
        if how == "mapped":  # what the zero-copy path uploads: the two runs, back to back
            runs = f.windows(k0, cnt)
            assert [ln for _, ln in runs] == [cnt * N * 2] * 2
            got = np.concatenate([np.ctypeslib.as_array((np.ctypeslib.ctypes.c_int8 * ln).from_address(a)) for a, ln in runs])
        else:
            dst = np.full(2 * 2 * N * 2 + 64, 0x5A, dtype=np.uint8)  # a slot sized for whole batches
            f.read_into(k0, cnt, dst, how=how)
            assert np.all(dst[nbytes:] == 0x5A)  # nothing beyond the batch's bytes
            got = dst[:nbytes].view(np.int8)
        half = cnt * N * 2
        assert np.array_equal(got[:half].reshape(cnt, N, 2), want[:, 0])  # the x plane ...
        assert np.array_equal(got[half:].reshape(cnt, N, 2), want[:, 1])  # ... then the y plane, one upload
    assert np.array_equal(f.cpi(4), want_batch(x, y, 4, 1, sx=3, sy=7)[0])
    for bad in ((5, 1), (4, 2), (-1, 1)):
        with pytest.raises(IndexError):
            f.extent(*bad)
    with pytest.raises(IndexError):
        f.cpi(5)
    with pytest.raises(ValueError):
        f.read_into(0, 2, np.zeros(100, dtype=np.uint8))
    f.close()


def test_cs8pair_threaded_read_and_lengths(tmp_path):
    """A batch large enough for the reader threads' split, and the CPI count of every length combination."""
    from concurrent.futures import ThreadPoolExecutor
    n = 1 << 20
    px, py, x, y = write_pair(tmp_path, 3 * n + 5, 3 * n, seed=4)
    f = R.Cs8Pair(px, py, n, skip_x=5)
    assert f.n_cpis == 3
    dst = np.zeros(2 * 3 * n * 2, dtype=np.uint8)
    with ThreadPoolExecutor(3) as pool:
        for how in ("memmove", "pread"):
            dst[:] = 0
            f.read_into(0, 3, dst, pool, 3, how)
            assert np.array_equal(dst[:3 * n * 2].view(np.int8).reshape(-1, 2), x[5:5 + 3 * n])
            assert np.array_equal(dst[3 * n * 2:].view(np.int8).reshape(-1, 2), y[:3 * n])
    f.close()
    for nx, ny, sx, sy, want in ((3000, 3000, 0, 0, 3), (3000, 2999, 0, 0, 2), (3999, 3000, 0, 0, 3), (3000, 3000, 1, 0, 2),
                                 (3000, 3000, 0, 1001, 1), (500, 3000, 0, 0, 0), (3000, 3000, 4000, 0, 0), (0, 0, 0, 0, 0)):
        a, b, _, _ = write_pair(tmp_path, nx, ny, odd_x=True)
        g = R.Cs8Pair(a, b, N, sx, sy)
        assert g.n_cpis == want, (nx, ny, sx, sy)
        g.close()
    with pytest.raises(ValueError):
        R.Cs8Pair(a, b, 0)
    with pytest.raises(ValueError):
        R.Cs8Pair(a, b, N, skip_x=-1)


def test_open_capture_and_layout(tmp_path):
    px, py, x, y = write_pair(tmp_path, 2 * N, 2 * N)
    f = R.open_capture(px, N, "cs8", path_y=py, skip_y=1)
    assert isinstance(f, R.Cs8Pair) and f.n_cpis == 1 and np.array_equal(f.cpi(0)[1], y[1:N + 1])
    f.close()
    with pytest.raises(ValueError):
        R.open_capture(px, N, "cs8")  # one file is not an 8-bit capture
    with pytest.raises(ValueError):
        R.open_capture(px, N, "rspduo", path_y=py)
    with pytest.raises(ValueError):
        R.open_capture(px, N, "cu8", path_y=py)
    for kind in ("HackRF", "Kraken", "hackrf", "KRAKEN"):
        assert R.capture_layout({"capture": {"device": {"type": kind}}}) == "cs8"
        assert R.config_layout({"capture": {"device": {"type": kind}}}) == "cs8"
    assert R.capture_layout({"capture": {"device": {"type": "Usrp"}}}) == "usrp"
    assert R.capture_layout({"capture": {"device": {"type": "RspDuo"}}}) == "rspduo"
    assert R.capture_layout({"capture": {"fs": 1}}) == "rspduo"


def stub(batch):
    # order-revealing per-CPI summary of int8 [2, n, 2] CPIs
    return [{"noisePower": float(np.abs(c[0].astype(np.float64)).mean()), "maxPower": float(c[1].astype(np.float64).sum())}
            for c in batch]


def test_single_process_cs8_replay(tmp_path):
    px, py, x, y = write_pair(tmp_path, 5 * N + 10, 5 * N)
    f = R.Cs8Pair(px, py, N)
    res = R.replay(f, stub, batch=2)
    assert [r["cpi"] for r in res] == list(range(5))
    want = stub(want_batch(x, y, 0, 5))
    assert [(r["noisePower"], r["maxPower"]) for r in res] == [(w["noisePower"], w["maxPower"]) for w in want]


def _worker(rank, world, port, px, py, batch, out_path):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = R.replay(R.Cs8Pair(px, py, N, skip_y=2), stub, batch=batch, dist=dist)
        if rank == 0:
            np.save(out_path, np.array([[r["cpi"], r["noisePower"], r["maxPower"]] for r in res]))
        else:
            assert res is None
    finally:
        dist.destroy_process_group()


def test_two_rank_cs8_replay_gloo(tmp_path):
    import torch.multiprocessing as mp
    px, py, x, y = write_pair(tmp_path, 7 * N, 7 * N + 2, seed=8)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res.npy")
    mp.spawn(_worker, args=(2, port, px, py, 2, out), nprocs=2, join=True)
    got = np.load(out)
    assert got[:, 0].astype(int).tolist() == list(range(7))  # every CPI once, file order
    want = stub(want_batch(x, y, 0, 7, sy=2))
    assert np.array_equal(got[:, 1], [w["noisePower"] for w in want])
    assert np.array_equal(got[:, 2], [w["maxPower"] for w in want])


def write_config(path, device_type):
    cap = {"fs": N}
    if device_type is not None:
        cap["device"] = {"type": device_type}
    yaml.safe_dump({"capture": cap,
                    "process": {"data": {"cpi": 1.0},
                                "ambiguity": {"delayMin": -10, "delayMax": 100, "dopplerMin": -100, "dopplerMax": 100},
                                "detection": {"enable": False}, "clutter": {"enable": False}}}, open(path, "w"))


class _StubChain:
    def __init__(self):
        self.seen = []

    def __call__(self, batch):
        self.seen.append(batch)
        return stub(batch)

    def close(self):
        pass


@pytest.fixture
def stub_chain(monkeypatch):
    made = {}

    def fake(cfg, device=0, batch=1, want_map=False, **kw):
        made.update(kw, cfg=cfg, batch=batch)
        made["chain"] = _StubChain()
        return made["chain"]
    monkeypatch.setattr(R, "gpu_processor", fake)
    return made


@pytest.mark.parametrize("device_type,args", [("HackRF", []), ("Kraken", []), ("RspDuo", ["--format", "cs8"])])
def test_cli_cs8(tmp_path, capsys, stub_chain, device_type, args):
    cfg = str(tmp_path / "config.yml")
    write_config(cfg, device_type)
    px, py, x, y = write_pair(tmp_path, 3 * N + 1, 3 * N + 1)
    R.main([px, "--capture-y", py, "-c", cfg, "--batch", "2", "--skip-x", "1", *args])
    assert stub_chain["layout"] == "cs8"
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().split("\n")]
    assert [r["cpi"] for r in lines] == [0, 1, 2]
    assert [r["maxPower"] for r in lines] == [w["maxPower"] for w in stub(want_batch(x, y, 0, 3, sx=1))]
    seen = stub_chain["chain"].seen
    assert [b.shape for b in seen] == [(2, 2, N, 2), (1, 2, N, 2)] and seen[0].dtype == np.int8


def test_cli_cs8_argument_errors(tmp_path, capsys, stub_chain):
    cfg = str(tmp_path / "config.yml")
    write_config(cfg, "HackRF")
    px, py, _, _ = write_pair(tmp_path, 2 * N, 2 * N)
    with pytest.raises(SystemExit) as e:
        R.main([px, "-c", cfg])
    assert e.value.code != 0 and "--capture-y" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        R.main([px, "--capture-y", py, "-c", cfg, "--skip-y", "-3"])
    with pytest.raises(SystemExit):
        R.main([px, "--capture-y", py, "-c", cfg, "--usrp-block", "363"])
    write_config(cfg, "RspDuo")
    with pytest.raises(SystemExit):  # a second file for a .rspduo capture is a mistake, not ignored
        R.main([px, "--capture-y", py, "-c", cfg])
    with pytest.raises(SystemExit):
        R.main([px, "-c", cfg, "--skip-x", "4"])
    assert "chain" not in stub_chain  # nothing was built


def test_abi_codes_and_symbol():
    """The two new format codes, in the header and in the binding, and the host-plane entry point in both."""
    import blah2_amd
    hdr = open(os.path.join(ROOT, "include", "blah2hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define BLAH2HIP_(FMT_\w+) (\d+)", hdr)}
    assert codes == {"FMT_C32": 0, "FMT_I16": 1, "FMT_F16": 2, "FMT_I16X_C32Y": 3, "FMT_I8": 4, "FMT_I8X_C32Y": 5}
    assert (_lib.FMT_I8, _lib.FMT_I8X_C32Y) == (4, 5) == (blah2_amd.FMT_I8, blah2_amd.FMT_I8X_C32Y)
    assert (_lib.FMT_C32, _lib.FMT_I16, _lib.FMT_F16, _lib.FMT_I16X_C32Y) == (0, 1, 2, 3)  # existing codes keep their values
    assert re.search(r"\bint\s+blah2hip_amb_process_i8\s*\(", hdr) and "blah2hip_amb_process_i8" in _lib.SYMBOLS
    assert "HackRf.cpp:119-127" in hdr and "Kraken.cpp:100-108" in hdr and "SIGNED" in hdr


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu8") / "emulate_i8")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "emulate_i8.cpp")])
    return exe


# (R3, nCorr, nPulses, delayMin, nDelay, nSeg, segLen)
@pytest.mark.parametrize("case", [
    (4, 4761, 3, -11, 112, 9, 576),     # odd nCorr, odd negative first lag, the 576-sample segments of the carried windows
    (4, 1541, 2, 1, 299, 3, 606),       # odd nCorr, positive (odd) first lag: a one-sided window
    (4, 1541, 2, -299, 299, 3, 606),    # the other side: delayMax = -1, every window starts below the pulse
    (8, 3899, 2, -9, 410, 3, 1300),     # odd nCorr at the configs[1] shape
    (8, 1001, 3, 3, 98, 1, 1001),       # one ragged segment, positive first lag
    (16, 9767, 2, -23, 2047, 5, 2049),  # half-zero x segments of the 4096-point kernel
    (4, 37, 5, -1, 3, 1, 37),           # tiny pulse
])
def test_i8_segment_windows_on_the_host(emu, case):
    out = subprocess.run([emu, *[str(v) for v in case], "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.match(r"mismatches=0 checked=(\d+)", out.stdout)
    assert m and int(m.group(1)) > 16 * 16 * case[0] * case[2], out.stdout
