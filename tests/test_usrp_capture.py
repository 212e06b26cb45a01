"""CPU suite: USRP captures (Usrp.cpp:96-104: per recv(), B complex<float> of the reference channel, then B of the
surveillance channel) -- the reader's layout, its raw batch ranges, the CPI sharding over it and the replay CLI's
choice of layout.  The device de-blocking is tests/test_usrp_replay_gpu.py."""
import json
import os
import socket

import numpy as np
import pytest
import yaml

from blah2_amd import replay as R

N = 1000  # samples per CPI: none of the blocks below but 1 divides it


def write_usrp(path, x, y, block, tail=b""):
    """The capture Usrp::process writes: block pair by block pair, every block full (the last one padded with zeros,
    the writer's stale values), then ``tail`` (a ragged end that holds no whole block pair).  Returns the two channels
    as the file holds them, padding included."""
    B = int(block)
    nb = -(-len(x) // B)
    xs = np.zeros(nb * B, dtype=np.complex64)
    ys = np.zeros(nb * B, dtype=np.complex64)
    xs[:len(x)], ys[:len(y)] = x, y
    with open(path, "wb") as f:
        for p in range(nb):
            f.write(xs[p * B:(p + 1) * B].tobytes())
            f.write(ys[p * B:(p + 1) * B].tobytes())
        f.write(tail)
    return xs, ys


def rand_c64(rng, n, scale=1000.0):
    return (rng.standard_normal(n) * scale + 1j * rng.standard_normal(n) * scale).astype(np.complex64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("block", [1, 7, 363, 2040, N + 5])
def test_usrp_file_layout(tmp_path, block):
    rng = np.random.default_rng(block)
    total = 5 * N + 321
    x, y = rand_c64(rng, total), rand_c64(rng, total)
    p = str(tmp_path / "a.usrp.iq")
    # the ragged tail: one x block of a pair whose y block never came, and a few bytes
    xs, ys = write_usrp(p, x, y, block, tail=rand_c64(rng, block).tobytes() + b"\x01\x02\x03")
    f = R.UsrpFile(p, N, block)
    assert f.n_cpis == len(xs) // N  # whole block pairs only; the padded last block counts, the tail does not
    assert f.n_cpis >= 5
    for k in range(f.n_cpis):
        c = f.cpi(k)
        assert c.shape == (2, N) and c.dtype == np.complex64
        assert np.array_equal(bits(c[0]), bits(xs[k * N:(k + 1) * N]))
        assert np.array_equal(bits(c[1]), bits(ys[k * N:(k + 1) * N]))
    b = f.batch(range(1, 4))
    assert b.shape == (3, 2, N)
    assert np.array_equal(bits(b), bits(np.stack([f.cpi(k) for k in (1, 2, 3)])))
    assert f.batch([4, 0]).shape == (2, 2, N) and f.batch([]).shape == (0, 2, N)
    with pytest.raises(IndexError):
        f.cpi(f.n_cpis)
    with pytest.raises(IndexError):
        f.cpi(-1)
    with pytest.raises(IndexError):
        f.extent(f.n_cpis - 1, 2)
    raw = open(p, "rb").read()
    for k0, cnt in [(0, 1), (1, 2), (2, f.n_cpis - 2), (f.n_cpis - 1, 1)]:
        off, nb, first = f.extent(k0, cnt)
        p0, p1 = k0 * N // block, ((k0 + cnt) * N - 1) // block
        assert (off, nb, first) == (p0 * 16 * block, (p1 - p0 + 1) * 16 * block, k0 * N - p0 * block)
        assert nb <= cnt * N * 16 + 32 * block  # what GpuChain stages per batch
        want = raw[off:off + nb]
        addr, ln = f.window(k0, cnt)
        assert ln == nb and bytes((np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * ln).from_address(addr)))) == want
        for how in ("memmove", "pread"):
            dst = np.full(nb + 64, 0xAB, dtype=np.uint8)
            f.read_into(k0, cnt, dst, how=how)
            assert dst[:nb].tobytes() == want and np.all(dst[nb:] == 0xAB)
        # the NumPy de-block of exactly those bytes is the batch
        got = R.usrp_deblock(np.frombuffer(want, dtype=np.complex64), block, first, N, cnt)
        assert np.array_equal(bits(got), bits(f.batch(range(k0, k0 + cnt))))
    f.close()


def test_usrp_file_short_and_invalid(tmp_path):
    p = str(tmp_path / "s.usrp.iq")
    write_usrp(p, np.ones(N - 1, np.complex64), np.ones(N - 1, np.complex64), 7 * 11 * 13)  # one 1001-sample pair
    assert R.UsrpFile(p, N, 1001).n_cpis == 1
    write_usrp(p, np.ones(N - 1, np.complex64), np.ones(N - 1, np.complex64), 999)  # 999 samples: no CPI
    f = R.UsrpFile(p, N, 999)
    assert f.n_cpis == 0 and f.batch([]).shape == (0, 2, N)
    with pytest.raises(IndexError):
        f.cpi(0)
    open(p, "wb").close()
    assert R.UsrpFile(p, N, 7).n_cpis == 0
    for bad in (0, -3):
        with pytest.raises(ValueError):
            R.UsrpFile(p, N, bad)
    assert isinstance(R.open_capture(p, N, "usrp", 7), R.UsrpFile)
    with pytest.raises(ValueError):
        R.open_capture(p, N, "usrp")
    with pytest.raises(ValueError):
        R.open_capture(p, N, "hackrf")


def test_rspduo_extent():
    """The one method both readers share with the device chain: a .rspduo CPI is whole 8-byte records."""
    f = R.RspduoFile.__new__(R.RspduoFile)
    f.n_samples = 257
    assert f.extent(3, 2) == (3 * 257 * 8, 2 * 257 * 8, 0)


def test_gpu_chain_layout_arguments():
    """Checked before anything touches a device."""
    with pytest.raises(ValueError):
        R.GpuChain({}, layout="kraken")
    with pytest.raises(ValueError):
        R.GpuChain({}, layout="usrp")
    with pytest.raises(ValueError):
        R.GpuChain({}, layout="usrp", usrp_block=0)


def make_usrp_capture(path, n_cpis, block=363, extra=17):
    rng = np.random.default_rng(1234)
    total = n_cpis * N + extra
    return write_usrp(path, rand_c64(rng, total), rand_c64(rng, total), block)


def stub(batch):
    # order-revealing per-CPI summary of complex (x, y) CPIs
    return [{"noisePower": float(np.abs(c[0].astype(np.complex128)).mean()), "maxPower": float(c[1].real.max())}
            for c in batch]


def test_single_process_usrp_replay(tmp_path):
    p = str(tmp_path / "a.usrp.iq")
    make_usrp_capture(p, 5)
    f = R.UsrpFile(p, N, 363)
    n = f.n_cpis
    res = R.replay(f, stub, batch=2)
    assert [r["cpi"] for r in res] == list(range(n))
    for r in res:
        assert r["noisePower"] == stub(f.batch([r["cpi"]]))[0]["noisePower"]
        assert r["maxPower"] == stub(f.batch([r["cpi"]]))[0]["maxPower"]


def _worker(rank, world, port, path, batch, out_path):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = R.replay(R.UsrpFile(path, N, 363), stub, batch=batch, dist=dist)
        if rank == 0:
            np.save(out_path, np.array([[r["cpi"], r["noisePower"], r["maxPower"]] for r in res]))
        else:
            assert res is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_cpis,batch", [(7, 2), (4, 3)])
def test_two_rank_usrp_replay_gloo(tmp_path, n_cpis, batch):
    import torch.multiprocessing as mp
    p = str(tmp_path / "b.usrp.iq")
    make_usrp_capture(p, n_cpis)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res.npy")
    mp.spawn(_worker, args=(2, port, p, batch, out), nprocs=2, join=True)
    got = np.load(out)
    f = R.UsrpFile(p, N, 363)
    assert got[:, 0].astype(int).tolist() == list(range(f.n_cpis))  # every CPI once, file order
    want = stub(f.batch(range(f.n_cpis)))
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


def test_cli_usrp_needs_its_block(tmp_path, capsys, stub_chain):
    cfg = str(tmp_path / "config.yml")
    write_config(cfg, "Usrp")
    cap = str(tmp_path / "a.usrp.iq")
    make_usrp_capture(cap, 2)
    with pytest.raises(SystemExit) as e:
        R.main([cap, "-c", cfg])
    assert e.value.code != 0 and "--usrp-block" in capsys.readouterr().err
    write_config(cfg, "RspDuo")
    with pytest.raises(SystemExit):  # --format usrp over an RspDuo config: the block is still needed
        R.main([cap, "-c", cfg, "--format", "usrp"])
    with pytest.raises(SystemExit):  # a block for a .rspduo capture is a mistake, not ignored
        R.main([cap, "-c", cfg, "--usrp-block", "363"])
    assert "chain" not in stub_chain  # nothing was built


def test_cli_reads_the_layout_from_the_config(tmp_path, capsys, stub_chain):
    cfg = str(tmp_path / "config.yml")
    write_config(cfg, "Usrp")
    cap = str(tmp_path / "a.usrp.iq")
    make_usrp_capture(cap, 3)
    f = R.UsrpFile(cap, N, 363)
    R.main([cap, "-c", cfg, "--usrp-block", "363", "--batch", "2"])
    assert stub_chain["layout"] == "usrp" and stub_chain["usrp_block"] == 363
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().split("\n")]
    assert [r["cpi"] for r in lines] == list(range(f.n_cpis))
    assert [r["maxPower"] for r in lines] == [w["maxPower"] for w in stub(f.batch(range(f.n_cpis)))]
    seen = stub_chain["chain"].seen
    assert [b.shape for b in seen] == [(2, 2, N), (f.n_cpis - 2, 2, N)] and seen[0].dtype == np.complex64


@pytest.mark.parametrize("device_type,args", [("RspDuo", []), (None, []), ("Usrp", ["--format", "rspduo"])])
def test_cli_rspduo_layout(tmp_path, capsys, stub_chain, device_type, args):
    cfg = str(tmp_path / "config.yml")
    write_config(cfg, device_type)
    cap = str(tmp_path / "a.rspduo")
    np.random.default_rng(3).integers(-2000, 2000, size=(3 * N, 4), dtype=np.int16).tofile(cap)
    R.main([cap, "-c", cfg, *args])
    assert stub_chain["layout"] == "rspduo" and stub_chain["usrp_block"] is None
    assert len(capsys.readouterr().out.strip().split("\n")) == 3
    assert stub_chain["chain"].seen[0].dtype == np.int16


def test_config_layout():
    assert R.config_layout({"capture": {"device": {"type": "Usrp"}}}) == "usrp"
    assert R.config_layout({"capture": {"device": {"type": "RspDuo"}}}) == "rspduo"
    assert R.config_layout({"capture": {"fs": 2000000}}) == "rspduo"
