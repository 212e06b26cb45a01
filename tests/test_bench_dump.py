"""CPU: what `bench.py --dump-outputs DIR` writes (dump_outputs on host tensors; no GPU needed), and that the options exist."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _amb(nD, nC):
    return types.SimpleNamespace(delay=np.arange(-2, nC - 2), doppler=np.linspace(-10.0, 10.0, nD))


def test_dump_ambiguity_outputs(tmp_path):
    B, nD, nC = 6, 5, 7
    g = torch.Generator().manual_seed(0)
    out = torch.complex(torch.randn(B, nD, nC, generator=g), torch.randn(B, nD, nC, generator=g))
    met = torch.randn(B, 2, generator=g, dtype=torch.float64)
    bench.dump_outputs(np, torch, str(tmp_path), _amb(nD, nC), out, met)
    assert sorted(os.listdir(tmp_path)) == ["map.npy", "map_cpis.npy", "metrics.npy"]
    m, cpis = np.load(tmp_path / "map.npy"), np.load(tmp_path / "map_cpis.npy")
    assert m.dtype == np.float32 and m.shape == (B, nD, nC, 2)
    assert np.array_equal(cpis, np.arange(B, dtype=np.float64))
    assert np.array_equal(m[..., 0], out.real.numpy()) and np.array_equal(m[..., 1], out.imag.numpy())
    assert np.array_equal(np.load(tmp_path / "metrics.npy"), met.numpy())


def test_dump_samples_cpis_within_budget(tmp_path, monkeypatch):
    B, nD, nC = 9, 4, 4
    monkeypatch.setattr(bench, "DUMP_MAP_BYTES", 3 * nD * nC * 8)
    out = torch.zeros(B, nD, nC, dtype=torch.complex64)
    bench.dump_outputs(np, torch, str(tmp_path), _amb(nD, nC), out, torch.zeros(B, 2, dtype=torch.float64))
    assert np.array_equal(np.load(tmp_path / "map_cpis.npy"), [0.0, 4.0, 8.0])  # evenly spaced, first and last included
    assert np.load(tmp_path / "map.npy").shape == (3, nD, nC, 2)


def test_dump_full_chain_detections(tmp_path):
    import blah2_amd
    B, nD, nC, cap = 3, 5, 7, 8
    hits = torch.zeros(B, cap, 2, dtype=torch.float64)
    rec = hits.numpy().view(blah2_amd.HIT_DTYPE).reshape(B, cap)
    rec["row"][:, :2], rec["col"][:, :2], rec["snr"][:, :2] = [3, 1], [6, 2], [20.0, 10.0]
    cnt = torch.tensor([2, 0, 1], dtype=torch.int32)
    ok = torch.tensor([1, 0, 1], dtype=torch.int32)
    amb = _amb(nD, nC)
    bench.dump_outputs(np, torch, str(tmp_path), amb, torch.zeros(B, nD, nC, dtype=torch.complex64),
                       torch.zeros(B, 2, dtype=torch.float64), ok, hits, cnt, cap)
    assert np.array_equal(np.load(tmp_path / "filter_ok.npy"), [1.0, 0.0, 1.0])
    det = np.load(tmp_path / "detections.npy")
    assert det.dtype == np.float64
    # (cpi, delay, doppler, snr) in the reference's row-major order
    assert np.array_equal(det, [[0, 2 + amb.delay[0], amb.doppler[1], 10.0], [0, 6 + amb.delay[0], amb.doppler[3], 20.0],
                                [2, 6 + amb.delay[0], amb.doppler[3], 20.0]])


def test_bench_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
