"""GPU: the drop-in C++ class with taps per block -- WienerHopf(delayMin, delayMax, nSamples, 4)::process(IqData*, IqData*),
blah2_amd/host/test/test_clutter_blocks.cpp -- against the fp64 restatement's filtered channel (tests/clutter_blocks_ref.py),
written as flat records the way tests/test_host_cpp_gpu.py writes test_golden's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import clutter_blocks_ref as R
import clutter_crafted as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "blah2_amd", "host", "test", "test_clutter_blocks")


def write_record(path, x, y, dmin, dmax, blocks, ok, y_ref):
    with open(path, "wb") as f:
        f.write(b"B2CLBK01")
        f.write(struct.pack("<5q", x.shape[0], dmin, dmax, blocks, int(ok)))
        for a in (x, y, y_ref):
            a = np.ascontiguousarray(a, dtype=np.complex128)
            f.write(struct.pack("<q", a.size))
            f.write(a.tobytes())


def test_cpp_wiener_hopf_with_blocks(built_lib, tmp_path):
    assert os.path.exists(EXE), "host test program was not built"
    n, blocks, dmin, dmax = 8192, 4, -3, 13
    L = n // blocks
    x, y = cc.cpis_for(dmin, dmax, n, 1)[0]
    ok, y_ref, _, _, _ = R.wiener_hopf_blocks(x, y, dmin, dmax, blocks)
    assert ok.all()
    good = str(tmp_path / "blocks4.bin")
    write_record(good, x, y, dmin, dmax, blocks, True, y_ref)
    x0 = x.copy()
    x0[2 * L:3 * L] = 0  # block 2's matrix is not positive definite: process() returns false, y keeps its samples
    assert R.wiener_hopf_blocks(x0, y, dmin, dmax, blocks)[0].tolist() == [True, True, False, True]
    bad = str(tmp_path / "blocks4_failed_block.bin")
    write_record(bad, x0, y, dmin, dmax, blocks, False, y)
    out = subprocess.run([EXE, good, bad], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "OK" in out.stdout


def test_cpp_check_can_fail(built_lib, tmp_path):
    """The same program on a record whose expected channel is the UNFILTERED y: it must report it and exit non-zero."""
    n, blocks, dmin, dmax = 8192, 4, -3, 13
    x, y = cc.cpis_for(dmin, dmax, n, 1)[0]
    path = str(tmp_path / "blocks4_off.bin")
    write_record(path, x, y, dmin, dmax, blocks, True, y)
    out = subprocess.run([EXE, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "CHECK FAILED" in out.stdout and "emax" in out.stdout
