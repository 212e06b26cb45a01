"""Offline replay of blah2 captures (.rspduo, USRP and 8-bit pairs), CPI-sharded across GPUs.

The reference replays a capture by pushing int16 I1 Q1 I2 Q2 samples into the
two IqData FIFOs (src/capture/rspduo/RspDuo.cpp:150-179) and the processing
thread cuts non-overlapping CPIs of nSamples out of them (blah2.cpp:254-258):
CPI k is exactly file bytes [k*nSamples*8, (k+1)*nSamples*8); each CPI's
products are emitted as soon as it is done, in order (blah2.cpp:299-321).
Ambiguity, WienerHopf, CfarDetector1D and Map::set_metrics carry no state from
one CPI to the next, so the capture shards over the ranks with NO data-path
collective.

A USRP capture (``YYYYmmdd-HHMMSS.usrp.iq``, Usrp.cpp:96-104) holds fc32 values
in channel blocks: B complex<float> of the reference channel, then B of the
surveillance channel, and so on, with B = UHD's get_max_num_samps, which the
file does not record (:class:`UsrpFile` is told it).  A CPI starts and ends
mid-block, but a batch of consecutive CPIs is still one contiguous byte range
of whole block pairs; the device chain uploads that range as it is and one
kernel (blah2hip_deblock_c32_dev) writes the two complex-fp32 planes the rest
of the chain reads.  The reference itself cannot replay such a file
(``Usrp::replay`` is empty, Usrp.cpp:108-111).

The 8-bit receivers (HackRF, KrakenSDR / RTL-SDR) deliver one stream of int8
I, Q pairs per device (HackRf.cpp:116-133, Kraken.cpp:97-112); a recording of
such a pair is two files, one per channel (what ``hackrf_transfer -r`` writes
per board).  :class:`Cs8Pair` reads them, and the device chain uploads the
bytes as they lie on disk -- 2 bytes per sample and channel -- for the kernels
to read directly (BLAH2HIP_FMT_I8): no conversion on the host or the device.
The reference has no file writer or replay for these devices (``replay`` is
empty, HackRf.cpp:135-138, Kraken.cpp:114-117).

The unit of work is a BATCH of `batch` consecutive CPIs (one contiguous read,
one launch of the device chain).  Batch b belongs to rank b mod world; a ROUND
is `world` consecutive batches.  Only the per-CPI results (two doubles + the
detection list, and the map when JSON is wanted) travel: after each round the
ranks' results are gathered to rank 0, which emits them in file order -- so
output streams while the capture is still being processed and every rank
holds one round of results at most.

On a rank the batches flow through a pipeline (:class:`GpuChain`): reader
threads copy the next batch out of the memory-mapped file into a ring of pinned
host buffers (or, ``read_mode="mapped"``, only register its pages with the
device: no CPU copy), a copy stream uploads batch k+1 and brings back the
results of batch k-1 while the kernels of batch k run on the compute stream;
HIP events order the three.
At 16 MB of int16 per 1 s CPI the GPU needs 9 us for what PCIe needs 290 us to
deliver: a replay is bound by the host link, and the pipeline's job is to keep
that link busy (tools/replay_bench.py measures both).  A USRP CPI is twice the
bytes (fc32), so the same link carries half the CPIs per second.

`processor` is a :class:`GpuChain`, or -- for the CPU tests of the sharding,
which has no GPU dependency -- any callable that takes what the capture's
``batch()`` returns (int16 [B, nSamples, 4] for .rspduo, complex64 [B, 2,
nSamples] (x, y) for USRP, int8 [B, 2, nSamples, 2] (x, y; I, Q) for an 8-bit
pair) and returns a list of B result dicts.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
import time
import pickle
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterator, List, Optional, Tuple

import numpy as np

from .chain_plan import _key, plan_chain

BYTES_PER_SAMPLE = 8  # int16 I1 Q1 I2 Q2
FC32_BYTES = 8  # one complex<float> of a USRP capture
CS8_BYTES = 2  # one int8 I, Q pair of an 8-bit capture
PAGE = 4096
_MADV_POPULATE_READ = 22  # Linux 5.14+
_LIBC = C.CDLL(None, use_errno=True)
_LIBC.madvise.argtypes = [C.c_void_p, C.c_size_t, C.c_int]


class _RawCapture:
    """What the readers share: a file memory-mapped in ``_mm`` whose batches of consecutive CPIs are contiguous byte ranges
    (:meth:`extent`), read out by :meth:`read_into` or exposed in place by :meth:`window`."""

    layout = ""

    def extent(self, k0: int, count: int) -> Tuple[int, int, int]:
        """(file offset, bytes, first) of CPIs k0 .. k0+count-1: the contiguous byte range a batch is read as, and the index
        of CPI k0's first sample inside that range, counted in samples of one channel."""
        raise NotImplementedError

    def read_into(self, k0: int, count: int, dst: np.ndarray, pool: Optional[ThreadPoolExecutor] = None, parts: int = 8,
                  how: str = "memmove"):
        """CPIs k0 .. k0+count-1 (contiguous in the file) into the first bytes of ``dst`` (any writable buffer, e.g. a
        pinned one), split over ``pool``'s threads.  ``how="memmove"``: out of the shared mapping -- each thread has the
        kernel fill the page tables of its piece (madvise MADV_POPULATE_READ: 47 GB/s per thread, against a fault per 64 KB)
        and copies it with memmove (non-temporal stores for large sizes): 12.5 GB/s per thread on the MI355X host;
        ``how="pread"``: the kernel's copy_to_user, 9.5 GB/s per thread.  PCIe takes 57."""
        off0, nbytes, _ = self.extent(k0, count)
        if how == "pread":
            if self._fd is None:
                self._fd = os.open(self.path, os.O_RDONLY)
            mv = memoryview(dst).cast("B")[:nbytes]

            def rd(a, b):
                pos = a
                while pos < b:
                    got = os.preadv(self._fd, [mv[pos:b]], off0 + pos)
                    if got <= 0:
                        raise IOError(f"short read from {self.path} at {off0 + pos}")
                    pos += got
        else:
            src = self._mm.ctypes.data + off0
            dstp = dst.ctypes.data
            if dst.nbytes < nbytes:
                raise ValueError("destination smaller than the CPIs asked for")

            def rd(a, b):
                lo = (src + a) // PAGE * PAGE  # madvise wants a page-aligned start; a failure only means the copy faults the pages in
                _LIBC.madvise(lo, src + b - lo, _MADV_POPULATE_READ)
                C.memmove(dstp + a, src + a, b - a)

        if pool is None or parts <= 1 or nbytes < (1 << 22):
            rd(0, nbytes)
            return
        step = -(-nbytes // parts)
        step += -step % 4096
        futs = [pool.submit(rd, a, min(a + step, nbytes)) for a in range(0, nbytes, step)]
        for f in futs:
            f.result()

    def window(self, k0: int, count: int) -> Tuple[int, int]:
        """(address, bytes) of CPIs k0 .. k0+count-1 inside the read-only shared mapping of the file: the page cache's own
        pages, which the zero-copy read path registers with the device and uploads from (``GpuChain(read_mode="mapped")``)."""
        off0, nbytes, _ = self.extent(k0, count)
        return self._mm.ctypes.data + off0, nbytes

    def windows(self, k0: int, count: int) -> List[Tuple[int, int]]:
        """The same as a list of (address, bytes) runs that land back to back in the batch's device buffer: one run for a
        capture that is one file."""
        return [self.window(k0, count)]

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None
        self._mm = np.zeros(0, dtype=self._mm.dtype)  # the mapping goes with its last reference (anything registered of it must be released first)


class RspduoFile(_RawCapture):
    """A .rspduo capture, indexed by CPI (memory-mapped for random access; :meth:`read_into` for streaming)."""

    layout = "rspduo"

    def __init__(self, path: str, n_samples: int):
        self.path = path
        self.n_samples = int(n_samples)
        size = os.path.getsize(path)
        self.n_cpis = size // (self.n_samples * BYTES_PER_SAMPLE)
        self._mm = np.memmap(path, dtype="<i2", mode="r") if size else np.zeros(0, dtype="<i2")
        self._fd = None

    def cpi(self, k: int) -> np.ndarray:
        if not 0 <= k < self.n_cpis:
            raise IndexError(k)
        a = self._mm[k * self.n_samples * 4:(k + 1) * self.n_samples * 4]
        return np.asarray(a).reshape(self.n_samples, 4)

    def batch(self, ks) -> np.ndarray:
        return np.stack([self.cpi(k) for k in ks]) if len(ks) else np.zeros((0, self.n_samples, 4), dtype=np.int16)

    def extent(self, k0: int, count: int) -> Tuple[int, int, int]:
        """CPI k is file bytes [k*nSamples*8, (k+1)*nSamples*8): whole records, ``first`` is 0."""
        return k0 * self.n_samples * BYTES_PER_SAMPLE, count * self.n_samples * BYTES_PER_SAMPLE, 0


def usrp_deblock(raw: np.ndarray, block: int, first: int, n_samples: int, n_cpi: int) -> np.ndarray:
    """complex64 [n_cpi, 2, n_samples]: (x, y) of CPI i, sample j = sample first + i*n_samples + j of each channel of
    ``raw``, the complex64 values of a USRP capture's byte range (blocks of ``block`` x samples, then ``block`` y
    samples: sample s of channel c is value (s // block) * 2*block + c*block + s % block).  The NumPy statement of
    blah2hip_deblock_c32_dev: an exact copy."""
    B = int(block)
    s = int(first) + np.arange(int(n_cpi) * int(n_samples), dtype=np.int64)
    at = (s // B) * (2 * B) + s % B
    out = np.empty((int(n_cpi), 2, int(n_samples)), dtype=np.complex64)
    out[:, 0] = raw[at].reshape(n_cpi, n_samples)
    out[:, 1] = raw[at + B].reshape(n_cpi, n_samples)
    return out


class UsrpFile(_RawCapture):
    """A USRP capture (Usrp.cpp:96-104: per recv(), ``block`` complex<float> of the reference channel x, then ``block`` of
    the surveillance channel y), indexed by CPI.  ``block`` is UHD's get_max_num_samps for the device and transport the
    capture was recorded with; the file does not record it.  Every block is taken as full: the writer pads a short
    recv() with stale values that the file cannot tell apart.  A trailing partial block pair belongs to no CPI.

    :meth:`cpi` and :meth:`batch` return complex64 [2, n] and [len, 2, n] (x, y); :meth:`read_into` and :meth:`window`
    give a batch's raw bytes (whole block pairs, :meth:`extent`), which the device chain de-blocks itself."""

    layout = "usrp"

    def __init__(self, path: str, n_samples: int, block: int):
        self.path = path
        self.n_samples = int(n_samples)
        self.block = int(block)
        if self.n_samples <= 0 or self.block <= 0:
            raise ValueError(f"UsrpFile: n_samples ({n_samples}) and block ({block}) must be positive")
        size = os.path.getsize(path)
        pairs = size // (2 * self.block * FC32_BYTES)
        self.n_cpis = pairs * self.block // self.n_samples
        self._mm = np.memmap(path, dtype=np.uint8, mode="r") if size else np.zeros(0, dtype=np.uint8)
        self._fd = None

    def extent(self, k0: int, count: int) -> Tuple[int, int, int]:
        """Whole block pairs floor(k0*n / B) .. floor(((k0+count)*n - 1) / B); ``first`` = k0*n mod B."""
        if k0 < 0 or count < 0 or k0 + count > self.n_cpis:
            raise IndexError((k0, count))
        n, B = self.n_samples, self.block
        p0 = k0 * n // B
        p1 = ((k0 + count) * n - 1) // B + 1 if count else p0
        return p0 * 2 * B * FC32_BYTES, (p1 - p0) * 2 * B * FC32_BYTES, k0 * n - p0 * B

    def batch(self, ks) -> np.ndarray:
        ks = list(ks)
        if not ks:
            return np.zeros((0, 2, self.n_samples), dtype=np.complex64)
        if ks == list(range(ks[0], ks[0] + len(ks))):  # consecutive (every batch replay() asks for): one pass
            off, nb, first = self.extent(ks[0], len(ks))
            return usrp_deblock(self._mm[off:off + nb].view("<c8"), self.block, first, self.n_samples, len(ks))
        return np.stack([self.cpi(k) for k in ks])

    def cpi(self, k: int) -> np.ndarray:
        if not 0 <= k < self.n_cpis:
            raise IndexError(k)
        return self.batch([k])[0]


class _Cs8Channel(_RawCapture):
    """One file of int8 I, Q pairs: CPI k is bytes [(skip + k*n)*2, (skip + (k+1)*n)*2)."""

    layout = "cs8"

    def __init__(self, path: str, n_samples: int, skip: int):
        self.path, self.n_samples, self.skip = path, int(n_samples), int(skip)
        size = os.path.getsize(path)
        self.pairs = size // CS8_BYTES  # an odd byte count: the dangling byte belongs to no sample
        self.n_cpis = max(0, self.pairs - self.skip) // self.n_samples
        self._mm = np.memmap(path, dtype=np.int8, mode="r") if size else np.zeros(0, dtype=np.int8)
        self._fd = None

    def extent(self, k0: int, count: int) -> Tuple[int, int, int]:
        return (self.skip + k0 * self.n_samples) * CS8_BYTES, count * self.n_samples * CS8_BYTES, 0


class Cs8Pair(_RawCapture):
    """An 8-bit capture: two files of int8 I, Q pairs, ``path_x`` the reference channel and ``path_y`` the surveillance
    channel -- the bytes the HackRF and KrakenSDR callbacks read (HackRf.cpp:119-127, Kraken.cpp:100-108: signed, I then
    Q), one stream per device, as ``hackrf_transfer -r`` or a signed-byte RTL-SDR dump writes them.  ``n_cpis`` is what
    BOTH files hold in whole CPIs: two boards never stop on the same sample, the tail of the longer file is ignored, and
    so is the dangling byte of an odd byte count.  Aligning the two streams is the capture's business, as in the
    reference, which starts the boards one after the other (HackRf.cpp:107-114); ``skip_x`` / ``skip_y`` drop that many
    leading samples of a channel for a user who knows the lag.

    :meth:`cpi` and :meth:`batch` return int8 [2, n, 2] and [len, 2, n, 2] (x, y; I, Q).  :meth:`read_into` puts a
    batch's x bytes, then its y bytes, back to back into the destination: the layout the device chain uploads and
    BLAH2HIP_FMT_I8 reads (x plane at byte 0, y plane at byte count * n * 2)."""

    layout = "cs8"

    def __init__(self, path_x: str, path_y: str, n_samples: int, skip_x: int = 0, skip_y: int = 0):
        self.n_samples = int(n_samples)
        if self.n_samples <= 0:
            raise ValueError(f"Cs8Pair: n_samples ({n_samples}) must be positive")
        if int(skip_x) < 0 or int(skip_y) < 0:
            raise ValueError("Cs8Pair: skip_x and skip_y are sample counts >= 0")
        self.path, self.path_y = path_x, path_y
        self._x = _Cs8Channel(path_x, self.n_samples, skip_x)
        self._y = _Cs8Channel(path_y, self.n_samples, skip_y)
        self.n_cpis = min(self._x.n_cpis, self._y.n_cpis)

    def _check(self, k0: int, count: int):
        if k0 < 0 or count < 0 or k0 + count > self.n_cpis:
            raise IndexError((k0, count))

    def extent(self, k0: int, count: int) -> Tuple[int, int, int]:
        """(0, bytes, 0): a batch is two byte ranges, one per file; ``bytes`` is their sum, the x half first."""
        self._check(k0, count)
        return 0, 2 * count * self.n_samples * CS8_BYTES, 0

    def read_into(self, k0, count, dst, pool=None, parts=8, how="memmove"):
        self._check(k0, count)
        half = count * self.n_samples * CS8_BYTES
        flat = np.frombuffer(memoryview(dst).cast("B"), dtype=np.uint8)
        if flat.nbytes < 2 * half:
            raise ValueError("destination smaller than the CPIs asked for")
        self._x.read_into(k0, count, flat[:half], pool, parts, how)
        self._y.read_into(k0, count, flat[half:2 * half], pool, parts, how)

    def window(self, k0: int, count: int):
        raise NotImplementedError("an 8-bit pair is two mappings: windows()")

    def windows(self, k0: int, count: int) -> List[Tuple[int, int]]:
        self._check(k0, count)
        return [self._x.window(k0, count), self._y.window(k0, count)]

    def batch(self, ks) -> np.ndarray:
        n = self.n_samples
        out = np.empty((len(ks), 2, n, 2), dtype=np.int8)
        for i, k in enumerate(ks):
            if not 0 <= k < self.n_cpis:
                raise IndexError(k)
            for c, ch in enumerate((self._x, self._y)):
                a = (ch.skip + k * n) * CS8_BYTES
                out[i, c] = np.asarray(ch._mm[a:a + n * CS8_BYTES]).reshape(n, 2)
        return out

    def cpi(self, k: int) -> np.ndarray:
        return self.batch([k])[0]

    def close(self):
        self._x.close()
        self._y.close()


def open_capture(path: str, n_samples: int, layout: str = "rspduo", usrp_block: Optional[int] = None,
                 path_y: Optional[str] = None, skip_x: int = 0, skip_y: int = 0) -> _RawCapture:
    """The reader for a capture of ``layout``: "rspduo", "usrp" (with its block length) or "cs8" (``path`` the reference
    channel's file, ``path_y`` the surveillance channel's)."""
    if layout == "cs8":
        if path_y is None:
            raise ValueError("an 8-bit capture is two files: path_y names the surveillance channel's")
        return Cs8Pair(path, path_y, n_samples, skip_x, skip_y)
    if path_y is not None:
        raise ValueError(f"path_y belongs to an 8-bit ('cs8') capture, not to layout {layout!r}")
    if layout == "rspduo":
        return RspduoFile(path, n_samples)
    if layout == "usrp":
        if usrp_block is None:
            raise ValueError("a USRP capture needs its block length (UHD's get_max_num_samps)")
        return UsrpFile(path, n_samples, usrp_block)
    raise ValueError(f"capture layout {layout!r}: 'rspduo', 'usrp' or 'cs8'")


class LoopedCapture(RspduoFile):
    """A capture read ``times`` times over, end to end, as ONE stream of ``times * n_cpis`` CPIs (throughput measurements
    that must last seconds from a file that fits /dev/shm: CPI k is CPI k mod n of the file).  A batch must not straddle
    the wrap: the file's CPI count has to be a multiple of the batch."""

    def __init__(self, path: str, n_samples: int, times: int):
        super().__init__(path, n_samples)
        self.n_file = self.n_cpis
        self.n_cpis = self.n_file * max(1, int(times))

    def _fold(self, k0: int, count: int) -> int:
        k = k0 % self.n_file
        if k + count > self.n_file:
            raise ValueError(f"batch [{k0}, {k0 + count}) straddles the end of a {self.n_file}-CPI capture read cyclically")
        return k

    def cpi(self, k: int) -> np.ndarray:
        if not 0 <= k < self.n_cpis:
            raise IndexError(k)
        k %= self.n_file
        return np.asarray(self._mm[k * self.n_samples * 4:(k + 1) * self.n_samples * 4]).reshape(self.n_samples, 4)

    def read_into(self, k0, count, dst, pool=None, parts=8, how="memmove"):
        return super().read_into(self._fold(k0, count), count, dst, pool, parts, how)

    def window(self, k0, count):
        return super().window(self._fold(k0, count), count)


def page_split(addr: int, nbytes: int, parts: int, page: int = PAGE):
    """The byte range [addr, addr + nbytes) as (head, [whole-page pieces], tail): ``head`` and ``tail`` are the ragged
    ends (offset, length) relative to ``addr`` that do not fill a page, the pieces are at most ``parts`` page-aligned
    (offset, length) runs between them.  The pieces are what gets registered with the device (two neighbouring
    batches never share a page that way); the ends, under a page each, travel through a small pinned buffer."""
    end = addr + nbytes
    lo = min(-(-addr // page) * page, end)
    hi = max(end // page * page, lo)
    head = (0, lo - addr)
    tail = (hi - addr, end - hi)
    pieces = []
    pages = (hi - lo) // page
    if pages > 0:
        parts = max(1, min(int(parts), pages))
        per = -(-pages // parts)
        for k in range(0, pages, per):
            cnt = min(per, pages - k)
            pieces.append((lo - addr + k * page, cnt * page))
    return head, pieces, tail


def shard_cpis(n_cpis: int, rank: int, world: int) -> List[int]:
    """Round-robin over single CPIs (batch = 1): rank r owns CPIs r, r+world, r+2*world, ..."""
    return list(range(rank, n_cpis, world))


def shard_batches(n_cpis: int, batch: int, rank: int, world: int) -> List[Tuple[int, int]]:
    """(first CPI, count) of the batches rank ``rank`` owns: batch b = CPIs [b*batch, (b+1)*batch) goes to rank b % world."""
    n_batches = -(-n_cpis // batch) if n_cpis else 0
    return [(b * batch, min(batch, n_cpis - b * batch)) for b in range(rank, n_batches, world)]


def _iter_local(capture: _RawCapture, processor, mine) -> Iterator[List[dict]]:
    """Results of this rank's batches, one list per batch, in order."""
    if hasattr(processor, "run_batches"):  # the pipelined device chain
        yield from processor.run_batches(capture, mine)
        return
    for k0, cnt in mine:
        out = processor(capture.batch(range(k0, k0 + cnt)))
        if len(out) != cnt:
            raise RuntimeError("processor returned a different number of results than CPIs")
        yield [dict(r, cpi=k0 + i) for i, r in enumerate(out)]


def _host_group(dist):
    """A gloo group over the same ranks for host-resident bytes (the default group may be RCCL, whose tensors live in
    HBM): results leave the device on their owning rank, so the gather moves host buffers."""
    if dist.get_backend() == "gloo":
        return None  # the default group will do
    return dist.new_group(backend="gloo")


def _gather_bytes(dist, group, payload: bytes, rank: int, world: int) -> Optional[List[bytes]]:
    """One round's results as TENSORS: every rank's byte count first (one int64 each), then the payloads padded to the
    longest.  What travels is what the owning rank serialised; rank 0 receives buffers, it does not unpickle objects it
    then has to format."""
    import torch
    n = torch.tensor([len(payload)], dtype=torch.int64)
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    longest = max(int(v.item()) for v in sizes)
    buf = torch.zeros(max(longest, 1), dtype=torch.uint8)
    if payload:
        buf[:len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
    parts = [torch.zeros_like(buf) for _ in range(world)] if rank == 0 else None
    dist.gather(buf, parts, dst=0, group=group)
    if rank != 0:
        return None
    return [bytes(p[:int(sz.item())].numpy().tobytes()) for p, sz in zip(parts, sizes)]


def replay(capture: _RawCapture, processor, batch: int = 1, dist=None, limit: Optional[int] = None,
           emit: Optional[Callable[[dict], None]] = None, serialise: Optional[Callable[[dict], dict]] = None,
           stats: Optional[dict] = None) -> Optional[List[dict]]:
    """Processes every CPI of ``capture`` exactly once across the ranks of ``dist`` (a torch.distributed module with an
    initialised default group, or None for a single process).

    With ``emit``: rank 0 calls ``emit(result)`` for every CPI in file order, round by round, while later rounds are still
    being processed (bounded memory), and the function returns the number of CPIs on rank 0.  Without: the results are
    collected and returned as a list on rank 0 (tests, small captures).  Other ranks return None.

    ``serialise`` runs on the rank that OWNS a CPI, before the gather: it turns the processor's result (which may hold a
    16 MB map) into what rank 0 has to emit -- the JSON documents of blah2.cpp:299-321, say -- and must keep the "cpi"
    key.  Rank 0's work per foreign CPI is then a receive and a write.  ``stats`` (a dict) receives this rank's seconds
    spent serialising, in the gather and (rank 0) emitting."""
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    n = capture.n_cpis if limit is None else min(limit, capture.n_cpis)
    if hasattr(processor, "shard_check"):
        processor.shard_check(world)  # (an integrating chain: windows inside a batch, or one rank)
    mine = shard_batches(n, batch, rank, world)
    n_batches = n_batches_hint(n, batch)
    n_rounds = -(-n_batches // world) if n_batches else 0
    collected: Optional[List[dict]] = [] if (emit is None and rank == 0) else None
    expect = 0
    done = 0
    t_ser = t_gather = t_emit = 0.0
    group = _host_group(dist) if dist is not None else None

    def deliver(results: List[dict]):
        nonlocal expect, done, t_emit
        t0 = time.perf_counter()
        for r in results:
            if r["cpi"] != expect:
                raise RuntimeError(f"replay order: CPI {r['cpi']} arrived where {expect} was due")
            expect += 1
            done += 1
            if emit is not None:
                emit(r)
            else:
                collected.append(r)
        t_emit += time.perf_counter() - t0

    local = _iter_local(capture, processor, mine)
    for g in range(n_rounds):
        own = next(local) if g * world + rank < n_batches else []
        if serialise is not None:
            t0 = time.perf_counter()
            own = [serialise(r) for r in own]
            t_ser += time.perf_counter() - t0
        if dist is None:
            deliver(own)
            continue
        t0 = time.perf_counter()
        parts = _gather_bytes(dist, group, pickle.dumps(own, protocol=pickle.HIGHEST_PROTOCOL) if own else b"", rank, world)
        t_gather += time.perf_counter() - t0
        if rank == 0:
            for part in parts:  # one round: `world` batches, rank order = file order
                deliver(pickle.loads(part) if part else [])
    if dist is not None:
        # a counter every rank agrees on (the throughput figure's numerator)
        import torch
        cnt = torch.tensor([sum(c for _, c in mine)], dtype=torch.int64)
        dist.all_reduce(cnt, group=group)
        if int(cnt.item()) != n:
            raise RuntimeError(f"replay processed {int(cnt.item())} CPIs, expected {n}")
    if stats is not None:
        stats.update(serialise_s=t_ser, gather_s=t_gather, emit_s=t_emit, cpis_owned=sum(c for _, c in mine))
    if rank != 0:
        return None
    if done != n:
        raise RuntimeError(f"replay emitted {done} CPIs, expected {n}")
    return done if emit is not None else collected


def n_batches_hint(n: int, batch: int) -> int:
    return -(-n // batch) if n else 0


def device_numa_cpus(torch, device: int = 0):
    """The CPUs of the NUMA node the GPU hangs off (sysfs, through the device's PCI address), or None when it cannot be told
    (one node, no sysfs, a container that hides it)."""
    try:
        bus = torch.cuda.get_device_properties(device).pci_bus_id  # torch >= 2.2
        dom = getattr(torch.cuda.get_device_properties(device), "pci_domain_id", 0)
        dev = getattr(torch.cuda.get_device_properties(device), "pci_device_id", 0)
        path = f"/sys/bus/pci/devices/{dom:04x}:{bus:02x}:{dev:02x}.0"
        node = int(open(path + "/numa_node").read())
        if node < 0:
            return None
        cpus = set()
        for part in open(f"/sys/devices/system/node/node{node}/cpulist").read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        return cpus or None
    except Exception:  # no device, no sysfs, an older torch: nothing to pin to
        return None


def pin_to_device_node(torch, device: int = 0) -> bool:
    """Run this thread -- and the threads it starts, and the pinned memory it allocates from now on -- on the GPU's NUMA
    node: the reader threads' copies then stay inside one socket's memory (a two-socket host moves them over the
    inter-socket links otherwise).  True if the affinity was changed."""
    cpus = device_numa_cpus(torch, device)
    if not cpus or cpus == os.sched_getaffinity(0):
        return False
    os.sched_setaffinity(0, cpus)
    return True


def _hip_runtime(torch):
    """libamdhip64 of the running torch, for hipHostRegister / hipHostUnregister / hipMemcpyAsync on raw addresses (torch
    has no tensor over read-only memory); None if it cannot be loaded."""
    try:
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        hip.hipHostRegister.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
        hip.hipHostUnregister.argtypes = [C.c_void_p]
        hip.hipSetDevice.argtypes = [C.c_int]
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipGetErrorString.restype = C.c_char_p
        return hip
    except OSError:
        return None


class GpuChain:
    """blah2.cpp:268-287 on the HIP engine for batches of CPIs, device resident from the int16 upload to the hit lists:
    clutter filter (optional; reads the .rspduo words directly) -> ambiguity -> metrics -> CFAR (blah2hip_cfar1d_dev),
    then Centroid and Interpolate when ``nCentroid`` is configured.  ``cfg`` carries the keys of the reference's config.yml
    ``process`` section plus ``fs`` and ``n_samples``.

    ``detect`` says where Centroid and Interpolate run.  "device" (the default when ``nCentroid`` is configured): one more
    kernel on the compute stream (blah2hip_detect_dev) on the hit lists and maps where they lie; the copy stream brings
    back the final records (32 bytes each) and their counts, the map stays on the device unless ``want_map`` asks for it,
    and collecting a batch makes no call into the library.  "host": the hit lists and every CPI's map come back and the
    host functions (blah2hip_centroid, blah2hip_interpolate) run per CPI.

    A ring of ``depth`` slots, each with a pinned host batch, its device copy, device result buffers and their pinned
    host copies.  For batch k: reader threads fill the slot's host buffer; the COPY stream uploads it; the COMPUTE stream
    (after the upload's event) runs the chain into the slot's result buffers; the copy stream (after the compute event)
    brings {metrics, ok flags, hit counts, the first ``hit_copy`` hit (or final) records per CPI, and the map when wanted} back.
    Batch k+1's read and upload and batch k-1's download overlap batch k's kernels.

    A CPI whose clutter filter fails (normal equations not positive definite) is SKIPPED like the reference does
    (``if (!filter->process(x, y)) continue;`` blah2.cpp:270-273): its result is ``{"skipped": True}``.

    ``layout`` is the capture layout the chain replays: "rspduo" (int16 I1 Q1 I2 Q2, read by the kernels as it is) or
    "usrp" with its block length ``usrp_block`` (:class:`UsrpFile`).  A USRP batch is uploaded as its raw bytes; on the
    compute stream blah2hip_deblock_c32_dev writes them into one pair of complex-fp32 planes [batch, n] (shared by the
    slots, like the filtered channel) and the FMT_C32 chain runs on those.  "cs8" replays a :class:`Cs8Pair`: a slot holds
    the batch's x bytes, then its y bytes, in one upload, and the kernels read the int8 pairs as they are (FMT_I8 into the
    filter and the range kernel, FMT_I8X_C32Y into the range kernel behind the filter): no conversion kernel, no fp32
    planes.  The filter of a cs8 chain is always the two-stage one (the fused kernel has no int8 form).

    ``cfg["integrate"] = {"window": W, "hop": H}`` (H optional, 1) puts a :class:`blah2_amd.MapIntegrator` behind the
    ambiguity stage on the compute stream: the detector (made for ``looks = W``) and the finisher run on the maps of the
    windows that end in the batch, and the result of CPI g is that window's -- its metrics, detections and (``want_map``)
    map, with ``"window": W`` -- or ``{"integrating": True}`` where no window ends at g.  A window that holds a skipped
    CPI is itself ``{"skipped": True}``.  The CPI count and the history run on from batch to batch; :meth:`run_batches`
    starts a capture at count 0, :meth:`reset_integrator` does so for a caller of ``chain(iq)``.  Ranks that take the
    batches round-robin see no consecutive CPIs across a batch's end: :meth:`shard_check` then asks for H == W and a batch
    of whole windows, and every batch starts at count 0.  Without the key the chain is the one described above.

    ``cfg["integrate"]["tracks"] = {"fc": HZ, "rate": QMAX | {"max": QMAX, "step": S}}`` takes the window sums ALONG THE
    TRACKS of the echoes (``MapIntegrator.set_tracks`` / ``process_tracks_dev``): the walk in delay between CPIs for the
    carrier ``fc`` (``blah2_amd.nci_walk_table``, back-to-back CPIs) under the bank ``blah2_amd.rate_bank(QMAX, S)`` of
    Doppler drifts in rows per CPI -- without ``rate`` the bank {0}, the walk only.  The detector is made with
    ``looks = W`` and ``pfa / K`` for the K hypotheses (the union bound).  ValueError, naming the key: no ``fc`` or one that
    is not positive and finite, a bank above 16 rates, a table the library refuses.  The multi-rank rule is unchanged.
    Without the key nothing new is launched.

    ``cfg["detection"]["cfar"] = "os"`` (default "ca") builds :class:`blah2_amd.OsCfarDetector1D` at
    ``cfg["detection"]["rank"]`` (default 0.75) in the place of ``CfarDetector1D``, for the integrator's looks as well; the
    hit buffers, the finisher and the results are the same.  ``"goca"`` / ``"soca"`` build
    :class:`blah2_amd.GoCfarDetector1D` (greatest-of / smallest-of) there; their thresholds are made for one look per cell,
    so with ``integrate`` or several carriers the plan raises a ValueError that names ``detection.cfar``.

    ``cfg["detection"]["clutterMap"] = {"memory": T, "mode": "gate" | "detect"}`` puts a
    :class:`blah2_amd.ClutterMapDetector` of memory T CPIs (normalised, at the detector's pfa -- ``pfa / K`` behind a rate
    bank) on the buffers the detector reads.  ``gate`` (default): the configured detector runs as before, cmap_kernel writes
    the batch's exceed planes, and the gate keeps the hits whose cell exceeded its own history -- the finisher and the
    downloads read the gated list, so an echo that sits in one cell CPI after CPI stops being reported after the first
    frames and one that moves stays.  ``detect``: the clutter map's own hit list takes the detector's place.  The history
    runs on from batch to batch (a skipped CPI's map is absorbed like any other); :meth:`run_batches` starts a capture at
    age 0.  ValueError, naming ``detection.clutterMap``: a memory outside [1, 64], an unknown mode, detection not enabled,
    ``integrate`` configured (the thresholds are one-look), and -- from :meth:`shard_check` -- more than one rank (the
    batches go round-robin: no rank sees consecutive CPIs).  Without the key nothing is allocated or launched.

    ``cfg["ambiguity"]["window"]`` names a Doppler taper (``blah2_amd.doppler_taper``: hann, hamming, blackman,
    blackmanharris, nuttall, flattop; ``NAME:norm`` divides the taps by a_0): one stencil kernel directly behind the
    ambiguity stage on the compute stream (``Ambiguity.taper_dev``), and everything after it -- the integrator, the
    detector, the finisher, the downloaded maps and metrics -- reads the tapered buffers.  The stage holds no state.
    Without the key, or with ``none``, nothing is allocated or launched.

    ``cfg["ambiguity"]["migration"] = {"fc": HZ}`` compensates range migration for the carrier ``fc``
    (``Ambiguity.migration_table`` / ``migrate_dev``): one kernel directly behind the ambiguity stage on the compute stream,
    in front of the taper, rewrites the batch's maps and metrics in place from the range map that the ambiguity stage left on
    the handle (every configuration of this chain runs ``process_dev``, so there always is one); everything after it reads
    the result.  ValueError: no ``fc``, an ``fc`` that is not positive and finite, or a geometry whose outermost Doppler row
    walks more than BLAH2HIP_MAX_MIGRATION cells.  Without the key nothing is allocated or launched.

    ``cfg["ambiguity"]["dopplerRate"] = QMAX`` or ``{"max": QMAX, "step": S}`` runs the Doppler-rate bank
    ``blah2_amd.rate_bank(QMAX, S)`` (bins drifted over the CPI, at most 16 hypotheses; ``Ambiguity.set_rates`` /
    ``rate_bank_dev``) in place behind the ambiguity stage and in front of the taper: every cell becomes the strongest of the
    bank's de-chirped Doppler sums.  With ``migration`` configured too, its table is set on the handle and this one kernel
    sums along the walk as well, INSTEAD of ``migrate_dev`` (two stages would each overwrite the other).  The maximum over K
    hypotheses multiplies the false-alarm rate by at most K, so the detector is made with ``pfa / K`` (the union bound).
    ValueError, naming the key: a bank of more than 16 rates, a ``max`` or ``step`` that is not a finite number (``max`` >= 0,
    ``step`` > 0), a bank the library refuses (|q| above the Doppler bins).  Without the key nothing is launched.

    ``cfg["detection"]["clean"] = {"snr": dB, "echoes": E, "sideDelay": 1, "sideDoppler": 0, "loading": 1e-6}`` cancels strong
    echoes on the samples (``blah2_amd.EchoCanceller``): behind the finisher the detections of at least ``snr`` dB, ``echoes``
    at the most, become clusters of atoms, their amplitudes are fitted to the fp32 surveillance plane by least squares and
    their replicas subtracted in place, and everything from the ambiguity stage on runs a second time.  A result carries the
    second pass's map and metrics, the merged list (``blah2_amd.merge_clean_detections``: the cancelled echoes from pass 1,
    then pass 2's detections less their residuals) and ``cancelled``, their number.  A configured fused FIR runs as the
    two-stage filter so that the filtered plane exists.  ValueError, naming the key: values outside their ranges, no device
    finisher (no ``nCentroid``, or ``detect="host"``), ``integrate`` or ``clutterMap`` configured (either would absorb every
    CPI twice), no fp32 surveillance plane at that point (int16 or int8 words and no clutter filter).  Without the key
    nothing is allocated or launched.

    ``cfg["ddc"] = {"offset": HZ, "decimation": D, "taps": T, "cutoff": 0.8, "beta": 8}`` (``capture.ddc`` of the config,
    ``--ddc``) puts the digital down-converter in front: ``cfg["fs"]`` and ``cfg["n_samples"]`` stay the capture's, the reader
    cuts CPIs of ``n_samples`` as before, a batch's raw samples (a USRP batch's de-blocked planes) go through
    ``blah2_amd.Channelizer`` into one pair of fp32 planes, and everything above is built for ``fs / D`` and ``n_samples / D``
    and runs on them as an ``FMT_C32`` chain (``self.fs``, ``self.n``; ``self.fs_in``, ``self.n_in`` are the capture's).  A
    migration or track carrier becomes ``fc + offset``.  ``taps`` defaults to ``16 D`` (at most 1024).  The filter's history
    runs from batch to batch: ``run_batches`` resets it, wants consecutive batches, and ``shard_check`` refuses several ranks.
    ValueError, naming ``capture.ddc``: values outside their ranges, a decimation that does not divide ``fs`` and
    ``n_samples``.  Without the key nothing is allocated or launched.

    ``cfg["ddc"]["offset"]`` may be a LIST of up to 8 offsets (``--ddc OFF0,OFF1,...:D``): the carriers of one mast, summed
    non-coherently on one velocity axis.  A list of one entry is the scalar, bit for bit.  With several, ``cfg["fc"]``
    (``capture.fc``, the capture's centre frequency) is needed: carrier c's Doppler axis scales with ``fc + offset_c``.
    The down-converter writes ``[n_car][batch][n]`` planes from its one pass, the clutter filter and the ambiguity stage run
    over ``n_car * batch`` virtual CPIs (their handles are made for that many), the taper, if configured, runs on all of
    them, and ``Ambiguity.fuse_carriers_dev`` sums each CPI's ``n_car`` maps along the table of
    ``blah2_amd.carrier_ratios(fc, offsets)`` (``cfg["ddc"]["interp"]``: ``nearest``, the default, or ``linear``;
    ``--ddc-interp``) into one map on CARRIER 0's AXIS: the frames' Doppler values are its own.  The integrator, if
    configured, runs on the fused maps with one channel; the detector is made for ``n_car`` looks (``n_car * W`` behind
    the integrator).  The outermost rows of the axis are not covered by the carriers above carrier 0's frequency: a
    result carries ``"carriers": n_car`` and ``"covered": [lo, hi]``, the Doppler interval every carrier covers, and
    detections outside it are dropped.  A CPI is skipped when the clutter filter fails on any carrier.  ValueError, naming
    ``capture.ddc``: more than 8 offsets, equal offsets, no ``fc`` or an ``fc + offset`` that is not positive, an unknown
    ``interp``, a ratio outside [0.5, 2], and several carriers together with ``ambiguity.migration``,
    ``ambiguity.dopplerRate`` or ``integrate.tracks`` (their tables are built for one carrier), ``detection.clutterMap``
    (its thresholds are for one look), ``detection.clean`` or ``detect="host"``."""

    def __init__(self, cfg: dict, device: int = 0, batch: int = 1, want_map: bool = False, depth: int = 3,
                 reader_threads: int = 4, hit_copy: int = 4096, read_mode: str = "memmove", numa: bool = True,
                 layout: str = "rspduo", usrp_block: Optional[int] = None, detect: Optional[str] = None):
        p = self.plan = plan_chain(cfg, layout, usrp_block, detect, batch)  # every refusal the dictionary alone decides
        if read_mode not in ("memmove", "pread", "mapped"):
            raise ValueError("read_mode: 'memmove', 'pread' or 'mapped'")
        self.layout, self.usrp_block = p.layout, p.usrp_block
        self.batch, self.depth, self.want_map = p.batch, max(2, int(depth)), bool(want_map)
        import torch

        import blah2_amd
        self.torch, self.b2 = torch, blah2_amd
        # The host side of the ring on the GPU's NUMA node (EPYC 9575F x 2, tools/gpu_hostreg.py: a reader thread copies
        # 17-19 GB/s inside the node, 12.5 when the scheduler puts it on the other socket; four threads 51-54 GB/s against
        # 41): the chain's OWN threads pin themselves when they start, and the pinned buffers are allocated (first touch)
        # with the calling thread on the node for the length of that allocation only -- the caller's affinity is what it
        # was when the constructor returns (a host program that builds chains for several devices, or has threads of its
        # own, is not narrowed to the last GPU's node).
        self._node_cpus = device_numa_cpus(torch, device) if numa else None
        self.numa_pinned = bool(self._node_cpus)
        self._handles = []  # (handle, whether close() closes it) in the order made: _own
        try:
            with self._on_node():
                self._make_handles(cfg, device)
                self._make_streams(device, hit_copy, read_mode)
                self._make_slots()
        except BaseException:  # whatever was made so far, last first (the integrator before its ambiguity handle)
            for h, _ in reversed(self._handles):
                h.close()
            raise
        # the threads last: nothing above leaves one running when it fails
        self.reader_threads = max(1, reader_threads)
        self.pool = ThreadPoolExecutor(max_workers=self.reader_threads, initializer=self._pin_worker)
        self._bg = ThreadPoolExecutor(max_workers=1, initializer=self._pin_worker)  # starts and awaits a batch's read while the main thread works on another

    def _own(self, handle, on_close=True):
        """Registers a handle the moment it exists; ``on_close``: :meth:`close` closes it (``amb`` and ``wh`` outlive that)."""
        self._handles.append((handle, on_close))
        return handle

    def _make_handles(self, cfg, device):
        """The plan as handles and detector objects, in the chain's order.  What only a handle can refuse: ValueError, naming the key."""
        p, b2, B = self.plan, self.b2, self.batch
        amb_c, det_c, clu_c = cfg["ambiguity"], cfg.get("detection") or {}, cfg.get("clutter") or {}
        self.fs_in, self.n_in, self.fs, self.n = p.fs_in, p.n_in, p.fs, p.n
        self.ddc_cfg, self.clean_cfg, self.clutter_blocks = p.ddc, p.clean, p.clutter["blocks"]
        self.taper = b2.doppler_taper_f32(*p.taper) if p.taper else None  # the Doppler taper's taps (None: no taper stage)
        # several carriers: the filter and the ambiguity stage see carrier c's CPI b as virtual CPI c * cnt + b
        self.n_car = n_car = len(p.carriers) if p.carriers else 1
        self.amb = amb = self._own(b2.Ambiguity(amb_c["delayMin"], amb_c["delayMax"], amb_c["dopplerMin"], amb_c["dopplerMax"],
                                                self.fs, self.n, True, device=device, max_batch=B * n_car), False)
        nD, nC = amb.get_n_doppler_bins(), amb.get_n_delay_bins()
        self.covered = None  # the Doppler interval every carrier covers (None: one carrier)
        if p.carriers:
            try:
                ratio = b2.carrier_ratios(p.carrier_fc, p.carriers)
                amb.set_carriers(ratio, p.carrier_interp)
                full = np.nonzero(amb.carrier_table(ratio, p.carrier_interp)["covered"] == n_car)[0]
            except (ValueError, b2.Blah2HipError) as e:
                raise ValueError(f"capture.ddc = {cfg['ddc']!r} at fc = {p.carrier_fc:g} Hz: {e}") from None
            self.covered = (float(amb.doppler[full[0]]), float(amb.doppler[full[-1]]))  # (carrier 0 covers every row)
        self.rates, self.migrate = p.rates, p.migrate_fc is not None
        if p.rates is not None:
            try:
                amb.set_rates(p.rates)
            except b2.Blah2HipError as e:
                raise ValueError(f"ambiguity.dopplerRate = {amb_c['dopplerRate']!r} on {nD} Doppler bins: {e}") from None
        if p.migrate_fc is not None:
            try:
                amb.set_migration(amb.migration_table(p.migrate_fc))
            except b2.Blah2HipError as e:
                raise ValueError(f"ambiguity.migration at fc = {p.migrate_fc:g} Hz: {e}") from None
        self.wh, self.fused_fir = None, False
        if p.clutter["enable"]:
            # a CPI has `blocks` flags, and is skipped when any block's matrix is not positive definite
            self.wh = self._own(b2.WienerHopf(clu_c["delayMin"], clu_c["delayMax"], self.n, device=device, max_batch=B * n_car,
                                              blocks=self.clutter_blocks), False)
            # the filter's FIR inside the range kernel where one 4096-point transform covers the geometry (range_fir_kernel):
            # the filtered channel never crosses HBM.  clutter: {fused: false} keeps the two-stage chain, and so do blocks
            # (the fused kernel takes one tap set per CPI: fir_fusable gives that reason) and clean (it needs the plane).
            self.fused_fir = p.clutter["fused"] and amb.fir_fusable(self.wh, p.fmt_in) is None
            if self.fused_fir:
                amb.set_fir(self.wh)
        if self.taper is not None and nD < 2 * (len(self.taper) - 1) + 1:
            raise ValueError(f"ambiguity.window {str(amb_c['window']).lower()!r}: a stencil of {2 * len(self.taper) - 1} taps "
                             f"on {nD} Doppler bins")
        self.nci, looks = None, {}
        if p.integrate:
            self.nci = self._own(b2.MapIntegrator(amb, 1, *p.integrate))  # (refuses a window outside [1, 16] or a hop of 0)
            # shard_check: every batch starts at count 0; CPIs handed over since the last reset; filter flags of the last W - 1 CPIs
            self._per_batch, self._g, self._ok_tail = False, 0, []
            looks = {"looks": self.nci.looks}
            if p.tracks:
                try:
                    self.nci.set_tracks(b2.nci_walk_table(amb, p.tracks[0]), p.tracks[1], max_cpi=B)
                except (ValueError, b2.Blah2HipError) as e:
                    raise ValueError(f"integrate.tracks = {cfg['integrate']['tracks']!r}: {e}") from None
        if p.carriers:  # a cell of the fused map is a sum of one look per carrier, times the integrator's window behind it
            looks = {"looks": n_car * looks.get("looks", 1)}
        self.nci_tracks = self.nci is not None and self.nci.n_rates > 0
        self.cfar = self.cmap = self.cmap_mode = self.centroid = self.interp = self.finisher = self.clean = self.ddc = None
        if p.cfar_kind:
            args = (p.pfa, det_c["nGuard"], det_c["nTrain"], det_c["minDelay"], det_c["minDoppler"])
            self.cfar = (b2.OsCfarDetector1D(*args, rank=p.rank, **looks) if p.cfar_kind == "os" else
                         b2.GoCfarDetector1D(*args, kind=p.cfar_kind[:2], **looks) if p.cfar_kind in ("goca", "soca") else
                         b2.CfarDetector1D(*args, **looks))  # all leave the same hit lists
            if p.cmap:
                self.cmap = self._own(b2.ClutterMapDetector(amb, p.pfa, p.cmap[0], det_c["minDelay"], det_c["minDoppler"]))
                self.cmap_mode = p.cmap[1]
            if p.centroid is not None:
                self.centroid = b2.Centroid(p.centroid, p.centroid, 1 / (self.n / self.fs))
                self.interp = b2.Interpolate(True, True)
        self.detect = p.detect  # where Centroid and Interpolate run (None: not configured)
        if p.detect == "device":
            self.finisher = b2.DetectionFinisher(self.centroid.nDelay, self.centroid.nDoppler, self.centroid.resolutionDoppler,
                                                 self.interp.doDelay, self.interp.doDoppler)
        self.need_map = self.want_map or p.detect == "host"
        self.cap = p.cap if p.cap is not None else min(nD * nC, 1 << 16)
        try:
            if p.clean:
                key = f"detection.clean = {det_c['clean']!r}"
                self.clean = self._own(b2.EchoCanceller(self.n, self.fs, amb_c["delayMin"], amb_c["delayMax"], device=device, max_batch=B))
            if p.ddc:  # every carrier from one pass, the history carried from batch to batch
                key = f"capture.ddc = {cfg['ddc']!r}"
                self.ddc = self._own(b2.Channelizer(self.fs_in, p.ddc["decimation"], p.ddc["h"],
                                                    list(p.carriers) if p.carriers else [p.ddc["offset"]], self.n_in,
                                                    max_rows=B, device=device))
        except b2.Blah2HipError as e:
            raise ValueError(f"{key}: {e}") from None

    def _make_streams(self, device, hit_copy, read_mode):
        """The two streams and what the slots share: the planes between the stages (the compute stream is in order)."""
        torch, B, n, n_in = self.torch, self.batch, self.n, self.n_in
        dev = self.dev = torch.device("cuda", device)
        self.hit_copy = min(self.cap, int(hit_copy))
        self.compute = torch.cuda.Stream(device=dev)
        self.copy = torch.cuda.Stream(device=dev)
        # How a batch gets from the page cache to the copy engine (tools/gpu_hostreg.py, tools/replay_bench.py; MI355X host):
        #   "memmove"  reader threads copy out of the file's shared mapping into a pinned ring (page tables filled by madvise
        #              first): 17-19 GB/s per thread on the GPU's NUMA node (12.5 across sockets), FOUR threads keep the link
        #              at 0.905 of its pinned rate (57 GB/s); three passes over DRAM
        #   "pread"    the same through the kernel's copy_to_user: 12.6 GB/s per thread on the node (9.5): 0.76 with four threads
        #   "mapped"   no CPU copy and ONE pass over DRAM: the threads only REGISTER whole-page pieces of the mapping with the
        #              device (hipHostRegister) and the copy engine reads the page cache's own pages.  A third to a half of the
        #              host CPU time -- but the driver registers 4 KB pages at 17-25 GB/s whatever the thread count (12-15 GB/s
        #              with the page-table fill of a first pass), so a replay that touches every page once gets 0.60 of the
        #              link from one thread and less from more.  For captures replayed repeatedly out of a mapping that stays
        #              (warm page tables) it reaches 0.94 of it with one thread.
        self._hip = _hip_runtime(torch) if read_mode == "mapped" else None
        self.read_mode = "memmove" if read_mode == "mapped" and self._hip is None else read_mode
        # the filtered surveillance channel
        self.yf = torch.empty((B * self.n_car, n), dtype=torch.complex64, device=dev) if self.wh is not None and not self.fused_fir else None
        # USRP: a batch's raw bytes are whole block pairs, at most B*n*16 + 32*block of them (a CPI run that starts and ends
        # mid-block); the de-blocked x and y planes are one pair for all slots, like yf
        self.raw_bytes = (-(-(B * n_in * 2 * FC32_BYTES + 4 * self.usrp_block * FC32_BYTES) // 16) * 16 if self.layout == "usrp" else
                          2 * B * n_in * CS8_BYTES if self.layout == "cs8" else None)  # cs8: the x bytes, then the y bytes
        self.planes = torch.empty((2, B, n_in), dtype=torch.complex64, device=dev) if self.layout == "usrp" else None
        # ... and so are the down-converter's output planes
        # (several carriers: carrier c's rows follow carrier c - 1's, cnt rows each, so a plane is a batch of n_car * cnt CPIs)
        self.ddc_planes = torch.empty((2, B * self.n_car, n), dtype=torch.complex64, device=dev) if self.ddc is not None else None
        self.busy_ms, self.batches_done = 0.0, 0  # kernels' time on the compute stream / batches collected, since construction

    def _make_slots(self):
        """The ring.  Each configured stage declares its device buffers, and with them the pinned host copies that come back:
        ``slot["down"]`` lists (host key, device key, records per row or None for all, rows per CPI or 0 for one per map) in
        the order ``_submit`` downloads them.  ``maps``, ``mets``, ``hits`` and ``cnt`` name the buffers that the stages behind
        the ambiguity stage, and the downloads, read: ``_submit`` points them at the last stage's."""
        torch, dev, B, cap, hc = self.torch, self.dev, self.batch, self.cap, self.hit_copy
        shape, A = (B, self.amb.get_n_doppler_bins(), self.amb.get_n_delay_bins()), self.b2._lib.MAX_ATOMS
        V = B * self.n_car  # virtual CPIs in front of the carrier sum (B with one carrier)
        vshape = (V,) + shape[1:]
        i32, f64, c64 = torch.int32, torch.float64, torch.complex64
        self.slots = []
        for _ in range(self.depth):
            s = {
                "h_iq": None,  # pinned staging batch of the pread path, allocated when that path first runs
                "h_ends": torch.empty(4 * PAGE, dtype=torch.uint8).pin_memory(),  # the ragged ends of a mapped batch's (one or two) runs
                "registered": [],
                "d_iq": torch.empty((B, self.n_in, 4), dtype=torch.int16, device=dev) if self.layout == "rspduo" else
                        torch.empty(self.raw_bytes, dtype=torch.uint8, device=dev),
                "first": 0,  # the batch's first sample inside its raw bytes (UsrpFile.extent)
                "h_hits": None, "h_map": None, "down": [],
                "uploaded": torch.cuda.Event(), "downloaded": torch.cuda.Event(),
                # the two ends of the batch's kernels on the (in-order) compute stream, timed: their sum over a replay is the
                # time the GPU spent computing (`busy_ms`), the rest of the wall clock it waited for the host link
                "started": torch.cuda.Event(enable_timing=True), "computed": torch.cuda.Event(enable_timing=True),
            }

            def stage(bufs, *down, **names):
                s.update({k: torch.zeros(sh, dtype=dt, device=dev) for k, (sh, dt) in bufs.items()})
                s.update({name: s[k] for name, k in names.items()})
                for h, d, cols, per in down:
                    shape_h = s[d].shape if cols is None else (B, cols) + s[d].shape[2:]
                    s[h] = torch.zeros(shape_h, dtype=s[d].dtype).pin_memory()
                    s["down"].append((h, d, cols, per))

            stage({"d_map": (vshape, c64), "d_met": ((V, 2), f64)}, ("h_met", "mets", None, 0), maps="d_map", mets="d_met")
            if self.wh is not None:  # the filter's flags, one per block (and carrier)
                stage({"d_ok": ((V * self.clutter_blocks,), i32)}, ("h_ok", "d_ok", None, self.n_car * self.clutter_blocks))
                s["d_ok"].fill_(1)
            if self.taper is not None:  # the tapered maps and their metrics: what everything behind the ambiguity stage reads
                stage({"d_tmap": (vshape, c64), "d_tmet": ((V, 2), f64)})
            if self.n_car > 1:  # the carriers' maps summed on carrier 0's axis: one map per CPI again
                stage({"d_fmap": (shape, c64), "d_fmet": ((B, 2), f64)}, maps="d_fmap", mets="d_fmet")
            if self.nci is not None:  # the integrated maps and their metrics: what the detector and the download read
                stage({"d_imap": (shape, c64), "d_imet": ((B, 2), f64)})
                s["nci"] = (0, 0, 0)  # (count before the batch, windows that end in it, count at which the first ends)
            if self.cfar is not None:  # blah2hip_hit_t records, 16 bytes; the count also for the capacity check
                stage({"d_hits": ((B, cap, 2), f64), "d_cnt": ((B,), i32)}, ("h_cnt", "cnt", None, 0),
                      hits="d_hits", cnt="d_cnt")  # the list the finisher and the downloads read
            if self.cmap_mode == "gate":  # the exceed planes, the gated list; the gated count never passes the capacity: the check needs the detector's own
                stage({"d_exc": (shape, torch.uint8), "d_ghits": ((B, cap, 2), f64), "d_gcnt": ((B,), i32)}, ("h_rcnt", "d_cnt", None, 0))
            if self.finisher is not None:  # blah2hip_det_t records, 32 bytes, as many as the hit list may hold (Centroid only drops)
                stage({"d_dets": ((B, cap, 4), f64), "d_dcnt": ((B,), i32)}, ("h_dcnt", "d_dcnt", None, 0), ("h_dets", "d_dets", hc, 0))
            elif self.cfar is not None:  # detect="host", or no nCentroid: the first hit_copy hits
                stage({}, ("h_hits", "hits", hc, 0))
            if self.clean is not None:  # pass 1's final list, the atoms (blah2hip_atom_t, 16 bytes) made of it, the fit; what _collect merges
                stage({"d_dets1": ((B, cap, 4), f64), "d_dcnt1": ((B,), i32), "d_atoms": ((B, A, 2), f64), "d_acnt": ((B,), i32),
                       "d_used": ((B, A), i32), "d_amp": ((B, A, 2), f64), "d_cok": ((B,), i32)},
                      ("h_dcnt1", "d_dcnt1", None, 0), ("h_dets1", "d_dets1", hc, 0), ("h_used", "d_used", None, 0), ("h_cok", "d_cok", None, 0))
            if self.need_map:
                stage({}, ("h_map", "maps", None, 0))
            self.slots.append(s)

    def _pin_worker(self):
        if self._node_cpus:
            try:
                os.sched_setaffinity(0, self._node_cpus)  # the calling thread only
            except OSError:
                pass

    @contextlib.contextmanager
    def _on_node(self):
        """The calling thread on the GPU's node for the length of a ``with`` block (pinned allocations), then back."""
        prev = None
        if self._node_cpus:
            try:
                prev = os.sched_getaffinity(0)
                os.sched_setaffinity(0, self._node_cpus)
            except OSError:
                prev = None
        try:
            yield
        finally:
            if prev is not None:
                os.sched_setaffinity(0, prev)

    def _fmt_in(self):
        """The format the filter and the range kernel read: .rspduo words, int8 planes, or the de-blocked or down-converted planes."""
        return self.plan.fmt_in

    def _host_batch(self):
        """The pinned staging batch of the copying read paths."""
        with self._on_node():
            if self.layout == "rspduo":
                return self.torch.empty((self.batch, self.n_in, 4), dtype=self.torch.int16).pin_memory()
            return self.torch.empty(self.raw_bytes, dtype=self.torch.uint8).pin_memory()

    def _check_capture(self, capture):
        layout = getattr(capture, "layout", "rspduo")
        if layout != self.layout:
            raise ValueError(f"a {self.layout} chain was handed a {layout} capture")
        if layout == "usrp" and capture.block != self.usrp_block:
            raise ValueError(f"USRP capture of block {capture.block} handed to a chain built for block {self.usrp_block}")

    # -- the three stages of one batch -------------------------------------------------
    def _read(self, capture: _RawCapture, slot: dict, k0: int, cnt: int):
        slot["mapped"] = None
        _, slot["nbytes"], slot["first"] = capture.extent(k0, cnt)
        if self.read_mode == "mapped":
            hip, dev = self._hip, self.dev.index
            # one run of the file per mapping (two for an 8-bit pair), landing back to back in the device buffer
            runs, at = [], 0
            for addr, nbytes in capture.windows(k0, cnt):
                runs.append((addr, at) + page_split(addr, nbytes, self.reader_threads))
                at += nbytes
            todo = [addr + o for addr, _, _, pieces, _ in runs for o, _ in pieces]
            lens = [ln for _, _, _, pieces, _ in runs for _, ln in pieces]

            def register(pc):
                hip.hipSetDevice(dev)  # the pool's threads start on device 0
                return hip.hipHostRegister(pc[0], pc[1], 0)

            rcs = list(self.pool.map(register, zip(todo, lens)))
            done = [a for a, rc in zip(todo, rcs) if rc == 0]
            if len(done) == len(todo):
                ends = slot["h_ends"].numpy()
                for r, (addr, _, head, _, tail) in enumerate(runs):
                    for (o, ln), e in ((head, 2 * r), (tail, 2 * r + 1)):  # under a page each: a copy
                        if ln:
                            C.memmove(ends.ctypes.data + e * PAGE, addr + o, ln)
                slot["registered"] = todo
                slot["mapped"] = runs
                return
            for a in done:
                hip.hipHostUnregister(a)
            self.read_mode = "memmove"  # this runtime / this file system does not register file mappings
            print(f"[blah2_amd.replay] hipHostRegister of the mapped capture failed ({hip.hipGetErrorString(max(rcs)).decode()}): "
                  "copying into a pinned buffer instead", file=sys.stderr)
        if slot["h_iq"] is None:
            slot["h_iq"] = self._host_batch()
        capture.read_into(k0, cnt, slot["h_iq"].numpy(), self.pool, self.reader_threads, how=self.read_mode)

    def _release(self, slot: dict):
        """The pieces of the mapping registered for this slot's batch (its upload has completed)."""
        for p in slot["registered"]:
            self._hip.hipHostUnregister(p)
        slot["registered"] = []

    def _submit(self, slot: dict, cnt: int):
        torch, b2, n, amb = self.torch, self.b2, self.n, self.amb
        with torch.cuda.stream(self.copy):
            if slot["mapped"] is not None:
                st, hip = self.copy.cuda_stream, self._hip
                ends = slot["h_ends"].data_ptr()
                for r, (addr, at, head, pieces, tail) in enumerate(slot["mapped"]):
                    dst = slot["d_iq"].data_ptr() + at
                    for src, (o, ln) in ([(addr + o, (o, ln)) for o, ln in pieces] +
                                         [(ends + 2 * r * PAGE, head), (ends + (2 * r + 1) * PAGE, tail)]):
                        if ln:
                            rc = hip.hipMemcpyAsync(dst + o, src, ln, 1, st)  # hipMemcpyHostToDevice
                            if rc:
                                raise RuntimeError(f"hipMemcpyAsync from the mapped capture: {hip.hipGetErrorString(rc).decode()}")
            elif self.layout == "rspduo":
                slot["d_iq"][:cnt].copy_(slot["h_iq"][:cnt], non_blocking=True)
            else:
                nb = slot["nbytes"]
                slot["d_iq"][:nb].copy_(slot["h_iq"][:nb], non_blocking=True)
            slot["uploaded"].record(self.copy)
        with torch.cuda.stream(self.compute):
            self.compute.wait_event(slot["uploaded"])
            slot["started"].record(self.compute)
            st = self.compute.cuda_stream
            iq = slot["d_iq"].data_ptr()
            if self.layout == "rspduo":  # the kernels read the .rspduo words
                fmt, fmt_yf, x, y = b2.FMT_I16, b2.FMT_I16X_C32Y, iq, None
            elif self.layout == "cs8":  # ... or the int8 pairs: the y plane follows the batch's x bytes
                fmt, fmt_yf, x, y = b2.FMT_I8, b2.FMT_I8X_C32Y, iq, iq + slot["nbytes"] // 2
            else:  # USRP: the batch's block pairs into the x and y planes first
                fmt, fmt_yf, x, y = b2.FMT_C32, b2.FMT_C32, self.planes[0].data_ptr(), self.planes[1].data_ptr()
                b2.deblock_c32_dev(iq, self.usrp_block, slot["first"], self.n_in, cnt, x, y, self.n_in, st)
            if self.ddc is not None:  # the batch's CPIs are consecutive rows of the stream; the chain reads the carrier's planes
                px, py_ = self.ddc_planes[0].data_ptr(), self.ddc_planes[1].data_ptr()
                self.ddc.process_dev(fmt, x, y, self.n_in, cnt, self.n_in, px, py_, n, cnt * n, st)
                fmt, fmt_yf, x, y = b2.FMT_C32, b2.FMT_C32, px, py_
            nv = cnt * self.n_car  # the virtual CPIs the filter and the ambiguity stage see: carrier c's CPI b is c * cnt + b
            if self.wh is None:
                amb.process_dev(fmt, x, y, nv, n, slot["d_map"].data_ptr(), slot["d_met"].data_ptr(), st)
            elif self.fused_fir:
                self.wh.estimate_dev_fmt(fmt, x, y, nv, n, slot["d_ok"].data_ptr(), st)
                amb.process_dev(fmt, x, y, nv, n, slot["d_map"].data_ptr(), slot["d_met"].data_ptr(), st)
            else:
                self.wh.process_dev_fmt(fmt, x, y, nv, n, self.yf.data_ptr(), n, slot["d_ok"].data_ptr(), st)
                amb.process_dev(fmt_yf, x, self.yf.data_ptr(), nv, n, slot["d_map"].data_ptr(),
                                slot["d_met"].data_ptr(), st)
            def behind(dets, dcnt):  # everything behind the ambiguity stage, on the maps it has just left; the final records into dets / dcnt
                n_maps, maps, mets = cnt, slot["d_map"], slot["d_met"]  # what the detector and the download read
                if self.rates is not None:  # in place too; along the migration table's walk when one is set: one sum for both
                    amb.rate_bank_dev(maps.data_ptr(), cnt, maps.data_ptr(), None, mets.data_ptr(), st)
                elif self.migrate:  # in place, from the range map the call above left on the handle
                    amb.migrate_dev(maps.data_ptr(), cnt, maps.data_ptr(), mets.data_ptr(), st)
                if self.taper is not None:
                    amb.taper_dev(maps.data_ptr(), nv, self.taper, slot["d_tmap"].data_ptr(), slot["d_tmet"].data_ptr(), st)
                    maps, mets = slot["d_tmap"], slot["d_tmet"]
                if self.n_car > 1:  # [n_car][cnt] maps into cnt, on carrier 0's Doppler axis
                    amb.fuse_carriers_dev(maps.data_ptr(), cnt, slot["d_fmap"].data_ptr(), slot["d_fmet"].data_ptr(), None, st)
                    maps, mets = slot["d_fmap"], slot["d_fmet"]
                if self.nci is not None:
                    if self._per_batch:
                        self.reset_integrator()
                    if self.nci_tracks:
                        n_maps, first = self.nci.process_tracks_dev(maps.data_ptr(), cnt, slot["d_imap"].data_ptr(), None,
                                                                    slot["d_imet"].data_ptr(), self.batch, None, st)
                    else:
                        n_maps, first = self.nci.process_dev(maps.data_ptr(), cnt, slot["d_imap"].data_ptr(), slot["d_imet"].data_ptr(),
                                                             self.batch, None, st)
                    slot["nci"] = (self._g, n_maps, first)
                    self._g += cnt
                    maps, mets = slot["d_imap"], slot["d_imet"]
                if self.cfar is not None and n_maps:
                    if self.cmap_mode == "detect":  # the clutter map's own list in the detector's place
                        self.cmap.process_dev(n_maps, slot["d_hits"].data_ptr(), self.cap, slot["d_cnt"].data_ptr(),
                                              maps.data_ptr(), mets.data_ptr(), None, None, st)
                    else:
                        self.cfar.process_dev(amb, n_maps, slot["d_hits"].data_ptr(), self.cap, slot["d_cnt"].data_ptr(),
                                              maps.data_ptr(), mets.data_ptr(), st)
                    if self.cmap_mode == "gate":  # the exceed planes, no list; then the detector's hits whose cell exceeded
                        self.cmap.process_dev(n_maps, None, 0, None, maps.data_ptr(), mets.data_ptr(), slot["d_exc"].data_ptr(), None, st)
                        self.cmap.gate_dev(slot["d_exc"].data_ptr(), n_maps, slot["d_hits"].data_ptr(), self.cap, slot["d_cnt"].data_ptr(),
                                           slot["d_ghits"].data_ptr(), slot["d_gcnt"].data_ptr(), st)
                        slot["hits"], slot["cnt"] = slot["d_ghits"], slot["d_gcnt"]
                    if self.finisher is not None:
                        self.finisher.process_dev(amb, n_maps, slot["hits"].data_ptr(), self.cap, slot["cnt"].data_ptr(),
                                                  dets.data_ptr(), self.cap, dcnt.data_ptr(),
                                                  maps.data_ptr(), mets.data_ptr(), st)
                slot["maps"], slot["mets"] = maps, mets
                return n_maps

            if self.clean is None:
                n_maps = behind(slot.get("d_dets"), slot.get("d_dcnt"))  # (None without a device finisher)
            else:
                # pass 1, its strongest detections as atoms, their replicas fitted to and taken out of the surveillance plane
                # (in place: the plane is this batch's alone on the in-order stream), then everything again: pass 2
                cc, A = self.clean_cfg, b2._lib.MAX_ATOMS
                behind(slot["d_dets1"], slot["d_dcnt1"])
                fy, py = (fmt_yf, self.yf.data_ptr()) if self.wh is not None else (fmt, y)
                self.clean.atoms_dev(amb, slot["d_dets1"].data_ptr(), self.cap, slot["d_dcnt1"].data_ptr(), cnt, cc["snr"], cc["echoes"],
                                     cc["sideDelay"], cc["sideDoppler"], slot["d_atoms"].data_ptr(), A, slot["d_acnt"].data_ptr(),
                                     slot["d_used"].data_ptr(), st)
                self.clean.process_dev(fy, x, py, cnt, n, slot["d_atoms"].data_ptr(), A, slot["d_acnt"].data_ptr(), cc["loading"],
                                       slot["d_amp"].data_ptr(), slot["d_cok"].data_ptr(), py, n, st)
                amb.process_dev(fy, x, py, cnt, n, slot["d_map"].data_ptr(), slot["d_met"].data_ptr(), st)
                n_maps = behind(slot["d_dets"], slot["d_dcnt"])
            slot["computed"].record(self.compute)
        with torch.cuda.stream(self.copy):
            self.copy.wait_event(slot["computed"])
            for h, d, cols, per in slot["down"]:  # every configured stage's pairs, as _make_slots declared them
                rows = cnt * per if per else n_maps
                slot[h][:rows].copy_(slot[d][:rows] if cols is None else slot[d][:rows, :cols], non_blocking=True)
            slot["downloaded"].record(self.copy)

    def _windows(self, slot: dict, ok_h, cnt: int):
        """The integrator's bookkeeping for one batch: ({c: at}, {c: skipped}) -- CPI c of the batch has a result where a
        window ends at it, the window's map is number ``at`` of the slot's buffers, and the window is skipped when the filter
        failed on any of its CPIs (the flags of the last W - 1 CPIs are kept for the next batch)."""
        g0, n_out, first = slot["nci"]
        W, H = self.nci.window, self.nci.hop
        if self._per_batch:
            self._ok_tail = []
        flags = self._ok_tail + [bool(v) for v in ok_h]  # flags[-cnt + c] is CPI c's
        at_of = {first - g0 + i * H: i for i in range(n_out)}
        skip_of = {c: not all(flags[len(flags) - cnt + c - W + 1:len(flags) - cnt + c + 1]) for c in at_of}
        self._ok_tail = flags[len(flags) - (W - 1):] if W > 1 else []
        return at_of, skip_of

    def _detections(self, slot: dict, b: int, r: dict):
        """The detections of map ``b`` of the slot into its record ``r``: the device finisher's list (merged with pass 1's
        behind CLEAN), or the hit list finished on the host."""
        b2, amb = self.b2, self.amb
        k = int(slot["h_cnt"][b])
        k_raw = int(slot["h_rcnt"][b]) if self.cmap_mode == "gate" else k
        if k_raw > self.cap:
            raise b2.Blah2HipError(b2._lib.ERR_CAPACITY, f"{k_raw} detections in one CPI, capacity {self.cap}")
        if self.finisher is None:
            if k > self.hit_copy:  # rare: more hits than the pipelined copy carries -- fetch this CPI's records now
                recs = slot["hits"][b, :k].cpu().numpy()
            else:
                recs = slot["h_hits"][b, :max(k, 1)].numpy()
            det = b2.hits_to_detection(amb, recs.view(b2.HIT_DTYPE).reshape(-1), k, self.cap)
            if self.centroid is not None:
                det = self.centroid.process(det)
                m = b2.Map(amb, slot["h_map"][b].numpy(), amb.delay, amb.doppler, r["noisePower"], r["maxPower"], b)
                det = self.interp.process(det, m)
            r.update(delay=det.get_delay().tolist(), doppler=det.get_doppler().tolist(), snr=det.get_snr().tolist())
            return

        def final(dets, dcnt):  # the final records, made on the device: sorted into emission order, no library call
            kd = int(slot["h_" + dcnt][b])
            if kd > self.cap:
                raise b2.Blah2HipError(b2._lib.ERR_CAPACITY, f"{kd} detections in one CPI, capacity {self.cap}")
            if kd > self.hit_copy:  # rare: beyond what the pipelined copy carries
                return slot["d_" + dets][b, :kd].cpu().numpy().view(b2.DET_DTYPE).reshape(-1), kd
            return slot["h_" + dets][b, :max(kd, 1)].numpy().view(b2.DET_DTYPE).reshape(-1), kd

        det = b2.dets_to_detection(*final("dets", "dcnt"), self.cap)
        if self.clean is None:
            r.update(delay=det.delay.tolist(), doppler=det.doppler.tolist(), snr=det.snr.tolist())
            return
        # the cancelled echoes from pass 1, then pass 2's list less their residuals
        first, k1 = final("dets1", "dcnt1")
        used = [int(u) for u in slot["h_used"][b].numpy() if u >= 0] if int(slot["h_cok"][b]) else []
        second = np.zeros(len(det.delay), dtype=b2.DET_DTYPE)
        second["delay"], second["doppler"], second["snr"] = det.delay, det.doppler, det.snr
        m = b2.merge_clean_detections(first[:k1], used, second, self.clean_cfg["sideDelay"], amb.dims.cpi)
        r.update(delay=m["delay"].tolist(), doppler=m["doppler"].tolist(), snr=m["snr"].tolist(), cancelled=len(used))

    def _collect(self, slot: dict, k0: int, cnt: int) -> List[dict]:
        slot["downloaded"].synchronize()
        self.busy_ms += slot["started"].elapsed_time(slot["computed"])
        self.batches_done += 1
        met_h = slot["h_met"].numpy()
        ok_h = (slot["h_ok"].numpy()[:self.n_car * cnt * self.clutter_blocks].reshape(self.n_car, cnt, self.clutter_blocks).all(axis=(0, 2))
                if self.wh is not None else np.ones(cnt, dtype=bool))  # (a CPI is skipped when the filter failed on any carrier)
        at_of, skip_of = (self._windows(slot, ok_h, cnt) if self.nci is not None else
                          ({c: c for c in range(cnt)}, {c: not ok_h[c] for c in range(cnt)}))
        res = []
        for c in range(cnt):
            if c not in at_of or skip_of[c]:
                res.append({"integrating" if c not in at_of else "skipped": True, "cpi": k0 + c})
                continue
            b = at_of[c]
            r = {"noisePower": float(met_h[b, 0]), "maxPower": float(met_h[b, 1]), "cpi": k0 + c}
            if self.nci is not None:
                r["window"] = self.nci.window
            if self.cfar is not None:
                self._detections(slot, b, r)
            if self.covered is not None:  # rows that not every carrier covers keep their looks of noise, but an echo there is not whole
                r.update(carriers=self.n_car, covered=list(self.covered))
                if "doppler" in r:
                    keep = [i for i, f in enumerate(r["doppler"]) if self.covered[0] <= f <= self.covered[1]]
                    r.update({k: [r[k][i] for i in keep] for k in ("delay", "doppler", "snr")})
            if self.want_map:
                r["map"] = slot["h_map"][b].numpy().copy()
            res.append(r)
        return res

    def run_batches(self, capture: _RawCapture, batches) -> Iterator[List[dict]]:
        """The pipeline over this rank's batches: yields each batch's results in order.  Up to ``depth`` batches are in
        flight; batch i's slot is reused by batch i + depth.  A slot has two halves with different lifetimes: its INPUT
        (the pinned batch, or the registered pages) is free as soon as the upload has completed, its RESULT buffers when the
        batch has been collected -- so the read of the next batch is started (on a background thread that drives the reader
        threads) the moment the previous read has ended, before this thread enqueues, synchronises, converts and yields:
        the reader threads never wait for Python.  A capture of another layout than the chain's is a ValueError."""
        self._check_capture(capture)
        self.reset_integrator()
        if self.cmap is not None:
            self.cmap.reset()  # a new capture: age 0
        batches = list(batches)
        if self.ddc is not None:  # a new capture: zero history, the stream's position at the first batch
            if any(a[0] + a[1] != b[0] for a, b in zip(batches, batches[1:])):
                raise ValueError("capture.ddc: the batches are not consecutive CPIs, so the down-converter's history does not carry")
            self.ddc.reset(batches[0][0] * self.n_in if batches else 0, self.compute.cuda_stream)
        D, n = self.depth, len(batches)
        reads = {}

        def start(j):
            slot = self.slots[j % D]
            slot["uploaded"].synchronize()  # the slot's previous upload (batch j - depth) is done with the input half
            self._release(slot)
            reads[j] = self._bg.submit(self._read, capture, slot, *batches[j])

        try:
            if n:
                start(0)
            for i in range(min(D - 1, n)):  # fill
                reads.pop(i).result()
                if i + 1 < n:
                    start(i + 1)
                self._submit(self.slots[i % D], batches[i][1])
            for i, (k0, cnt) in enumerate(batches):
                j = i + D - 1
                if j < n:
                    reads.pop(j).result()
                    if j + 1 < n:
                        start(j + 1)  # into the input half of the slot whose results are collected below
                    self._submit(self.slots[j % D], batches[j][1])
                yield self._collect(self.slots[i % D], k0, cnt)
        finally:
            for f in reads.values():  # a consumer that stopped early: let the read finish before its pages are released
                f.result()
            self.release_all()

    def __call__(self, iq: np.ndarray) -> List[dict]:
        """One batch, synchronously, from a host array [B, nSamples, 4] (tests; a caller that has the samples in memory).
        .rspduo chains only."""
        if self.layout != "rspduo":
            raise ValueError("GpuChain(...)(iq) takes .rspduo int16 samples; a USRP or cs8 chain replays its capture reader")
        cnt = iq.shape[0]
        slot = self.slots[0]
        if slot["h_iq"] is None:
            slot["h_iq"] = self._host_batch()
        slot["h_iq"][:cnt].copy_(self.torch.from_numpy(np.ascontiguousarray(iq)))
        slot["mapped"] = None
        self._submit(slot, cnt)
        out = self._collect(slot, 0, cnt)
        for r in out:
            r.pop("cpi", None)
        return out

    def reset_integrator(self):
        """The integrator (``cfg["integrate"]``) back at CPI count 0, its history forgotten; nothing without one.  Call it
        with no batch in flight."""
        if self.nci is not None:
            self.nci.reset()
            self._g, self._ok_tail = 0, []

    def shard_check(self, world: int):
        """:func:`replay` over ``world`` ranks deals the batches round-robin, so a rank does not see the CPIs in front of
        its batch: an integrating chain then needs windows that do not overlap and do not cross a batch's end (hop ==
        window, batch a multiple of the window), and starts every batch at count 0.  ValueError otherwise.  A clutter map
        needs every CPI in order, whatever the batch: more than one rank is a ValueError."""
        if self.plan.needs_order and world > 1:
            key, whose = ("detection.clutterMap", "a cell's") if self.cmap is not None else ("capture.ddc", "the filter's")
            raise ValueError(f"{key} over {world} ranks: the batches go round-robin, so no rank sees the "
                             f"consecutive CPIs {whose} history is made of")
        if self.nci is None or world <= 1:
            return
        W, H = self.nci.window, self.nci.hop
        if H != W or self.batch % W != 0:
            raise ValueError(f"integrate over {world} ranks: the batches go round-robin, so windows must not overlap or cross a "
                             f"batch's end: hop == window and batch % window == 0 (window {W}, hop {H}, batch {self.batch})")
        self._per_batch = True

    def release_all(self):
        """Unregister whatever is still registered (before the capture's mapping goes away)."""
        self.torch.cuda.synchronize(self.dev)
        for slot in self.slots:
            self._release(slot)

    def close(self):
        self._bg.shutdown(wait=True)
        self.pool.shutdown(wait=True)
        self.release_all()
        for h, on_close in self._handles:
            if on_close:
                h.close()


def gpu_processor(cfg: dict, device: int = 0, batch: int = 1, want_map: bool = False, **kw) -> GpuChain:
    """The device chain for :func:`replay` (kept under its old name)."""
    return GpuChain(cfg, device, batch, want_map, **kw)


def frames_for(result: dict, amb, fs: int, timestamp: int):
    """The two JSON documents blah2.cpp sends per CPI (:304-317): the map (``Map::to_json`` +
    ``delay_bin_to_km``) and the detections (``Detection::to_json`` + ``delay_bin_to_km``), produced by
    the C++ host classes (libblah2host.so, include/blah2host.h).  A document is one TCP "frame": the
    Node API appends chunks until the buffer ends with ``}`` (api/server.js:123-136)."""
    from . import _hostlib as H
    docs = {"map": H.map_json(result["map"], amb.delay, amb.doppler, result["noisePower"], result["maxPower"], timestamp, fs)}
    if "delay" in result:
        docs["detection"] = H.detection_json(result["delay"], result["doppler"], result["snr"], timestamp, fs)
    return docs


MTU = 1024  # src/process/utility/Socket.cpp:5


def send_frame(sock, doc: str):
    """Socket::sendData (Socket.cpp:21-32): the document in MTU-sized writes, no terminator."""
    raw = doc.encode("ascii")
    for i in range(0, len(raw), MTU):
        sock.sendall(raw[i:i + MTU])


def config_layout(y: dict) -> str:
    """The capture layout that goes with a blah2 config.yml: "usrp" for capture.device.type Usrp, "cs8" for the 8-bit
    receivers HackRF and Kraken (the spellings src/capture/Capture.cpp compares against, case-insensitive here; their
    drivers save nothing themselves: the layout is that of the bytes their callbacks read), else "rspduo" (the RspDuo's,
    and the default of a config that names no device)."""
    dev = ((y or {}).get("capture") or {}).get("device") or {}
    kind = str(dev.get("type", "")).lower()
    return "usrp" if kind == "usrp" else "cs8" if kind in ("hackrf", "kraken") else "rspduo"


capture_layout = config_layout


def main(argv=None):
    import argparse
    import socket

    import yaml
    ap = argparse.ArgumentParser(description="CPI-sharded replay of a blah2 capture (.rspduo, USRP or an 8-bit pair) on MI355X")
    ap.add_argument("capture", help="the capture; for --format cs8 the reference channel's file")
    ap.add_argument("-c", "--config", required=True, help="blah2 config.yml")
    ap.add_argument("--format", choices=("rspduo", "usrp", "cs8"), default=None,
                    help="capture layout (default: from the config's capture.device.type: Usrp, HackRF / Kraken (cs8) or RspDuo)")
    ap.add_argument("--capture-y", default=None, metavar="FILE",
                    help="cs8 captures: the surveillance channel's file of int8 I Q pairs (the positional capture is the "
                         "reference channel's)")
    ap.add_argument("--skip-x", type=int, default=0, metavar="S", help="cs8 captures: leading samples of the reference file to drop")
    ap.add_argument("--skip-y", type=int, default=0, metavar="S", help="cs8 captures: leading samples of the surveillance file to drop")
    ap.add_argument("--usrp-block", type=int, default=None, metavar="B",
                    help="USRP captures: samples per channel block, the get_max_num_samps UHD reported when the capture "
                         "was recorded (the file does not hold it)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--json", action="store_true",
                    help="emit, per CPI in file order, the map and detection documents blah2.cpp sends (one per line on "
                         "stdout, or as TCP frames with --connect)")
    ap.add_argument("--detect", choices=("device", "host"), default=None,
                    help="where Centroid and Interpolate run when detection.nCentroid is configured: in one kernel on the "
                         "hit lists and maps where they lie (device, the default), or on the host, which then downloads "
                         "every CPI's map")
    ap.add_argument("--clutter-blocks", type=int, default=None, metavar="B",
                    help="clutter filter with taps per block: cut each CPI into B equal blocks (overrides process.clutter.blocks "
                         "of the config; 1 = one tap set per CPI); the chain then runs the two-stage filter")
    ap.add_argument("--integrate", default=None, metavar="W[:H]",
                    help="non-coherent integration of the maps over a sliding window of W consecutive CPIs (1 ... 16), a "
                         "window every H CPIs (default 1); the detector's thresholds are made for W looks.  CPIs at which no "
                         "window ends give no frame.  Several ranks: H == W and --batch a multiple of W")
    ap.add_argument("--integrate-tracks", nargs="?", const=True, default=None, metavar="QMAX[:STEP]",
                    help="with --integrate: take the window sums along the echoes' tracks -- the walk in delay between CPIs "
                         "for the carrier capture.fc of the config, under the bank -QMAX ... QMAX of Doppler drifts in rows "
                         "per CPI in steps of STEP (default 1), at most 16 of them; without a value the walk only.  The "
                         "detector is made with W looks and pfa / K for the K hypotheses")
    ap.add_argument("--doppler-window", default=None, metavar="NAME[:norm]",
                    help="Doppler taper behind the ambiguity stage: none, hann, hamming, blackman, blackmanharris, nuttall or "
                         "flattop; :norm divides the taps by a_0 (an echo on a Doppler bin keeps its amplitude); overrides "
                         "process.ambiguity.window of the config")
    ap.add_argument("--migration", nargs="?", const=True, default=None, metavar="FC_HZ",
                    help="range-migration compensation behind the ambiguity stage (in front of the taper) for the carrier "
                         "FC_HZ; without a value the config's capture.fc.  process.ambiguity.migration: true in the config "
                         "does the same")
    ap.add_argument("--doppler-rate", default=None, metavar="QMAX[:STEP]",
                    help="Doppler-rate (acceleration) bank behind the ambiguity stage, in front of the taper: every cell becomes "
                         "the strongest of the hypotheses -QMAX ... QMAX in steps of STEP (default 1), in Doppler bins drifted "
                         "over the CPI, at most 16 of them; with --migration the same kernel sums along the range walk too.  The "
                         "maximum over K hypotheses multiplies the false-alarm rate by at most K, so the detector is made with "
                         "pfa / K (the union bound).  Overrides process.ambiguity.dopplerRate (QMAX or {max: QMAX, step: STEP})")
    ap.add_argument("--cfar", default=None, metavar="KIND[:RANK]",
                    help="the detector: ca (cell averaging, the reference's), goca / soca (greatest-of / smallest-of: the cell "
                         "against the mean of each half of its window, for clutter edges / for echoes in each other's window) "
                         "or os[:RANK] (ordered statistic: the threshold "
                         "from the RANK-th part of the sorted training cells, default 0.75); overrides "
                         "process.detection.cfar / .rank of the config")
    ap.add_argument("--clutter-map", default=None, metavar="T[:detect]",
                    help="a clutter-map CFAR of memory T CPIs (1 .. 64) behind the detector: every cell against the average "
                         "of its own past power, so what sits in one cell CPI after CPI is no longer reported.  T gates the "
                         "detector's hits, T:detect reports the clutter map's own.  One rank, not with --integrate.  "
                         "Overrides process.detection.clutterMap ({memory: T, mode: gate | detect})")
    ap.add_argument("--clean", default=None, metavar="SNR_DB[:MAX_ECHOES]",
                    help="strong-echo cancellation: the detections of at least SNR_DB (at most MAX_ECHOES of them, default 4) "
                         "are fitted to the surveillance samples by least squares and subtracted, and the chain runs again "
                         "from the ambiguity stage on; the frames carry the second pass's maps and the merged list.  Needs "
                         "device detection and an fp32 surveillance plane (a USRP capture or the clutter filter); not with "
                         "--integrate or --clutter-map.  Overrides process.detection.clean ({snr, echoes, sideDelay, "
                         "sideDoppler, loading})")
    ap.add_argument("--ddc-interp", choices=("nearest", "linear"), default=None,
                    help="several carriers (--ddc OFF0,OFF1,...:DECIM, at most 8; needs capture.fc): how a carrier's Doppler rows "
                         "are aligned with carrier 0's axis before the power maps are summed: the nearest row (default; the "
                         "detector's false-alarm rate holds exactly) or the two rows around it, weighted (loses less of an echo "
                         "between rows; the detector is conservative).  Overrides capture.ddc.interp")
    ap.add_argument("--ddc", default=None, metavar="OFFSET_HZ[,OFFSET_HZ...]:DECIM[:TAPS[:CUTOFF[:BETA]]]",
                    help="wideband captures: mix the carrier OFFSET_HZ off the capture's centre to zero, low-pass (a Kaiser-"
                         "windowed sinc of TAPS taps, default 16 DECIM and at most 1024, pass band CUTOFF of the output's "
                         "Nyquist rate, default 0.8, BETA default 8) and decimate by DECIM (1 .. 64, a divisor of capture.fs "
                         "and of the CPI's samples) on the device; everything behind runs at capture.fs / DECIM, and the "
                         "migration carrier becomes capture.fc + OFFSET_HZ.  Several offsets, at most 8, are the carriers of "
                         "one mast: their power maps are summed on the first one's Doppler axis (--ddc-interp), which needs "
                         "capture.fc and excludes --migration, --doppler-rate, --integrate-tracks, --clutter-map, --clean and "
                         "--detect host.  One rank.  Overrides capture.ddc ({offset, decimation, taps, cutoff, beta, interp})")
    ap.add_argument("--connect", action="store_true",
                    help="with --json: send the documents to network.ip:ports.map / ports.detection of the config, "
                         "framed like Socket::sendData, instead of printing them")
    # --ddc -16384,16384:4: a value that starts with a negative offset is no number to argparse, which would take it for an option
    argv, i = list(sys.argv[1:] if argv is None else argv), 0
    while i + 1 < len(argv):
        if argv[i] == "--ddc" and len(argv[i + 1]) > 1 and argv[i + 1][0] == "-" and argv[i + 1][1] in "0123456789.":
            argv[i:i + 2] = ["--ddc=" + argv[i + 1]]
        i += 1
    a = ap.parse_args(argv)
    y = yaml.safe_load(open(a.config))
    layout = a.format or config_layout(y)
    if layout == "usrp" and a.usrp_block is None:
        ap.error("a USRP capture needs --usrp-block B (UHD's get_max_num_samps for the device and transport it was "
                 "recorded with)")
    if a.usrp_block is not None and (layout != "usrp" or a.usrp_block <= 0):
        ap.error("--usrp-block takes a positive block length, for USRP captures only")
    if layout == "cs8" and a.capture_y is None:
        ap.error("an 8-bit (cs8) capture is two files: --capture-y FILE names the surveillance channel's")
    if layout != "cs8" and (a.capture_y is not None or a.skip_x or a.skip_y):
        ap.error("--capture-y, --skip-x and --skip-y belong to 8-bit (cs8) captures only")
    if a.skip_x < 0 or a.skip_y < 0:
        ap.error("--skip-x and --skip-y are sample counts >= 0")
    fs = int(y["capture"]["fs"])
    n = int(fs * float(y["process"]["data"]["cpi"]))  # blah2.cpp:142-144
    cfg = dict(y["process"], fs=fs, n_samples=n)
    if y["capture"].get("ddc"):
        cfg["ddc"] = dict(y["capture"]["ddc"])
    if y["capture"].get("fc") is not None:  # several carriers: their Doppler axes scale with capture.fc + offset
        cfg["fc"] = y["capture"]["fc"]

    def parsed(flag, form, names, convs, at_least=1, **defaults):
        """A flag's ``A:B:...`` as the dictionary its config key holds.  Syntax only: plan_chain below weighs the values."""
        parts = getattr(a, flag).split(":")
        try:
            if not at_least <= len(parts) <= len(names):
                raise ValueError
            return dict(defaults, **{k: conv(v) for k, conv, v in zip(names, convs, parts)})
        except ValueError:
            ap.error(f"--{flag.replace('_', '-')} takes {form}")

    def det_(**kw):
        return dict(cfg.get("detection") or {}, **kw)

    if a.ddc is not None:
        def offsets(v):  # OFF, or OFF0,OFF1,...: the list form of capture.ddc.offset
            return [float(f) for f in v.split(",")] if "," in v else float(v)

        cfg["ddc"] = parsed("ddc", "OFFSET_HZ[,OFFSET_HZ...]:DECIM[:TAPS[:CUTOFF[:BETA]]]", ("offset", "decimation", "taps", "cutoff", "beta"),
                            (offsets, int, int, float, float), 2,
                            **({"interp": cfg["ddc"]["interp"]} if (_key(cfg, "ddc") or {}).get("interp") is not None else {}))
    if a.ddc_interp is not None:
        if not _key(cfg, "ddc"):
            ap.error("--ddc-interp belongs to --ddc / capture.ddc")
        cfg["ddc"] = dict(cfg["ddc"], interp=a.ddc_interp)
    if a.clutter_blocks is not None:
        if a.clutter_blocks < 1:
            ap.error("--clutter-blocks takes a block count >= 1")
        cfg["clutter"] = dict(cfg.get("clutter") or {}, blocks=a.clutter_blocks)
    if a.integrate is not None:
        cfg["integrate"] = parsed("integrate", "W or W:H, a window and a hop in CPIs", ("window", "hop"), (int, int), hop=1)
        if min(cfg["integrate"].values()) < 1:
            ap.error("--integrate takes W or W:H, a window and a hop in CPIs, both >= 1")
    if a.integrate_tracks is not None:
        if not cfg.get("integrate"):
            ap.error("--integrate-tracks belongs to --integrate W[:H]")
        trk_ = {"fc": (_key(cfg["integrate"], "tracks") or {}).get("fc", y["capture"].get("fc"))}
        if trk_["fc"] is None:
            ap.error("--integrate-tracks needs a carrier: capture.fc in the config")
        if a.integrate_tracks is not True:
            trk_["rate"] = parsed("integrate_tracks", "QMAX or QMAX:STEP in Doppler rows per CPI", ("max", "step"), (float, float), step=1.0)
        cfg["integrate"] = dict(cfg["integrate"], tracks=trk_)
    if a.doppler_window is not None:
        cfg["ambiguity"] = dict(cfg["ambiguity"], window=a.doppler_window.lower())
    # process.ambiguity.migration: true, or --migration [FC_HZ]: the chain's {"fc": HZ}, the carrier from capture.fc by default
    mig_ = a.migration if a.migration is not None else cfg["ambiguity"].get("migration")
    if mig_:
        fc_ = mig_.get("fc") if isinstance(mig_, dict) else None if mig_ is True else mig_
        if fc_ is None:
            fc_ = y["capture"].get("fc")
        if fc_ is None:
            ap.error("range-migration compensation needs a carrier: --migration FC_HZ, or capture.fc in the config")
        try:
            cfg["ambiguity"] = dict(cfg["ambiguity"], migration={"fc": float(fc_)})
        except (TypeError, ValueError):
            ap.error("--migration takes a carrier frequency in Hz")
    elif "migration" in cfg["ambiguity"]:
        cfg["ambiguity"] = {k: v for k, v in cfg["ambiguity"].items() if k != "migration"}
    if a.doppler_rate is not None:
        cfg["ambiguity"] = dict(cfg["ambiguity"], dopplerRate=parsed("doppler_rate", "QMAX or QMAX:STEP in Doppler bins",
                                                                     ("max", "step"), (float, float), step=1.0))
    if a.cfar is not None:
        kind, _, rank_ = a.cfar.partition(":")
        try:
            if kind not in ("ca", "os", "goca", "soca") or (rank_ and (kind != "os" or not 0.001 <= float(rank_) <= 1.0)):
                raise ValueError
        except ValueError:
            ap.error("--cfar takes ca, goca, soca, os or os:RANK with RANK in [0.001, 1]")
        cfg["detection"] = det_(cfar=kind, **({"rank": float(rank_)} if rank_ else {}))
    if a.clutter_map is not None:
        cfg["detection"] = det_(clutterMap=parsed("clutter_map", "T or T:detect (T:gate is the default), T a memory of 1 .. 64 CPIs",
                                                  ("memory", "mode"), (int, str), mode="gate"))
    if a.clean is not None:
        cfg["detection"] = det_(clean=dict(_key(cfg.get("detection"), "clean") or {}, **parsed(
            "clean", "SNR_DB or SNR_DB:MAX_ECHOES, a threshold in dB and 1 .. 32 echoes", ("snr", "echoes"), (float, int), echoes=4)))
    try:  # everything the dictionary alone decides, before a process group or a device is touched
        plan = plan_chain(cfg, layout, a.usrp_block, a.detect, a.batch)
    except ValueError as e:
        ap.error(str(e))
    if plan.needs_order and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--ddc / capture.ddc and --clutter-map / detection.clutterMap need the CPIs in order: one rank")
    dist = None
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch
        import torch.distributed as dist_
        torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
        dist_.init_process_group("nccl" if torch.cuda.device_count() >= int(os.environ["WORLD_SIZE"]) else "gloo")
        dist = dist_
    import torch
    proc = gpu_processor(cfg, local % max(1, torch.cuda.device_count()), a.batch, want_map=a.json, layout=layout,
                         usrp_block=a.usrp_block, detect=a.detect)
    rank0 = dist is None or dist.get_rank() == 0
    socks = {}
    if rank0 and a.json and a.connect:
        ip = y["network"]["ip"]
        ip = "127.0.0.1" if ip == "0.0.0.0" else ip
        for name in ("map", "detection"):
            socks[name] = socket.create_connection((ip, int(y["network"]["ports"][name])))
    t_cpi_ms = int(round(1000.0 * n / fs))

    def serialise(r):  # on the rank that owns the CPI: Map::to_json + delay_bin_to_km there, documents on the wire
        if r.get("skipped") or r.get("integrating") or not a.json:
            return r
        # replay has no wall clock: CPI k is stamped k * tCpi in ms (blah2.cpp uses the capture time in ms)
        return {"cpi": r["cpi"], "frames": frames_for(r, proc.amb, proc.fs, r["cpi"] * t_cpi_ms)}

    def emit(r):  # rank 0, file order, as the rounds complete: a write per document
        if r.get("skipped") or (a.json and r.get("integrating")):
            return
        if not a.json:
            sys.stdout.write(json.dumps(r) + "\n")
            return
        for name, doc in r["frames"].items():
            if socks:
                send_frame(socks[name], doc)
            else:
                sys.stdout.write(doc + "\n")
        sys.stdout.flush()

    replay(open_capture(a.capture, n, layout, a.usrp_block, a.capture_y, a.skip_x, a.skip_y), proc, a.batch, dist, a.limit,
           emit=emit, serialise=serialise)
    for s in socks.values():
        s.close()
    proc.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
