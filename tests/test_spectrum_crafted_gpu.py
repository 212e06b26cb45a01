"""GPU: the spectrum analyser's kernels (blah2_amd/csrc/spectrum.hip) on the crafted rows and inputs of
tests/spectrum_crafted.py, through b2.SpectrumAnalyser.

Every device call writes [rows][nS] complex128 into an int32 allocation filled with a NaN-payload guard word, 64 guard words
behind it; the guard, and the rows a call must not write, are checked after every call.  Gate: spectrum_crafted.GATE on
err = max_k |got - ref| / rms_k(ref) against oracle.blah2_oracle.spectrum_process (A N in place of the rms where the
expectation is zero); tests/test_spectrum_crafted_model.py shows that every wrong term of the algebra misses it a thousand
times over.

Cases: 1. every row as a lone FMT_C32 CPI: impulses at 0, 1, nS - 1, nS, N - 1 (closed-form spectra), only the ignored tail
non-zero (the spectrum == 0), tones on bins 0, nS - 1 and either side of the rotation's wrap (argmax), a tone off the comb,
noise plus a tone over the int16 range; the host entry points (complex64, complex128) bit for bit the device call.  2. the
chunks of the fold on this device's compute units: ragged at D = 1003, empty at D = 5001 (at D = 16, as at any D, nJ <= D / 4
chunks of four or more leave none empty below D = (nJ - 1)^2: the empty chunks need the cap).  3. formats on four rows (the
smallest, staged, L2, chirp-z): int8-range samples as C32, I16 (.rspduo words, junk in tuner 2), F16 and I8 give identical
bits; I16 over +-32767 (and -32768); F16 with quarter steps.  4. batches of 1, 3, 4 of 4 on a row of each path, strides N,
N + 5 (junk between the CPIs) and n: every row bit for bit the lone call of the same handle, rows n_cpi .. 3 untouched; the
other formats once each at N + 5.  5. reuse: +-30000, then zeros (== 0), then the first CPI again (the first bits), with
nJ > 1 and on a chirp-z row.  6. refusals, with the codes of include/blah2hip.h, none of which writes the output.  7. the
wall time of nS = 65536, the last direct size.

FLOOR 3.5e-13 (folded_restatement against the reference on the CPU), GATE = 64 FLOOR = 2.24e-11.  The figure is set by tones: a
tone's own bin stands sqrt(nS) above the rms of the bins and carries eps sqrt(nS) of rounding, in the reference too (2.5e-13
from the long-double definition at nS = 131073); impulses and noise stay at 1e-15 on every row.

Measured on the MI355X, worst figure per path (C32, every input of every row): staged 7.1e-14 (nS = 4096, D = 3, tone on bin
0; 1.2e-14 and less below nS = 4096), L2 tables 2.3e-14 at nS = 4097 and 7.6e-13 at nS = 65536 (tone on bin 0; its noise 1.9e-13), chirp-z 5.4e-13
(nS = 131073, tone on bin 65535; 3.0e-13 .. 4.5e-13 on the other five rows).  Per format: I16 over the full range 2.6e-16 /
1.8e-15 / 8.4e-15 / 5.0e-14 and F16 quarter steps 3.5e-16 / 1.5e-15 / 3.6e-15 / 6.4e-15 on n7 / n1293 / l2-c3 / cz-fold; I16,
F16 and I8 of int8-range samples: the bits of the C32 call, lone and in batches.  nS = 65536, one CPI: 0.02 s wall with the
upload and the read-back, so the row runs every input like the others.  Nothing was found wrong in spectrum.hip.

Two things the rows showed about the chirp-z length, neither a defect: lags +-(nS - 1) of the conjugate chirp hold the same
value, so 2 nS - 2 points would do (nS = 65537 fits M = 131072); and the chirp of an even nS has period nS, so nS = 131072,
"the tightest wrap", would be exact on M = nS.  The planted `small-M` defect therefore shows on cz-tail and cz-mid only.
"""
import time

import numpy as np
import pytest

import spectrum_crafted as SC

pytestmark = pytest.mark.gpu

GUARD = np.uint32(0x7FC0BEEF)  # a NaN payload no kernel produces
PAD = 64
MAX_BATCH = 4
GAP = 5
FORMATS = ("c32", "i16", "f16", "i8")
FORMAT_ROWS = ("n7", "n1293", "l2-c3", "cz-fold")      # the smallest, staged (tail of 3), L2 tables, chirp-z behind a fold
BATCH_ROWS = ("n1293", "l2-c3", "cz-fold")
REUSE_ROWS = ("n10030", "cz-fold")


@pytest.fixture(scope="module")
def b2(built_lib):
    import blah2_amd
    assert blah2_amd.device_count() > 0
    return blah2_amd


@pytest.fixture(scope="module")
def handles(b2):
    """One handle per (row, max_batch) for the module: the chirp-z rows build their tables once."""
    made = {}

    def get(name, max_batch=1):
        if (name, max_batch) not in made:
            g = SC.BY_NAME[name]
            sa = b2.SpectrumAnalyser(g.n, g.bw, max_batch=max_batch)
            assert (sa.decimation, sa.nSpectrum, sa.nfft) == (g.D, g.nS, g.N)
            made[(name, max_batch)] = sa
        return made[(name, max_batch)]

    yield get
    for sa in made.values():
        sa.close()


def fmt_code(b2, fmt):
    return {"c32": b2.FMT_C32, "i16": b2.FMT_I16, "f16": b2.FMT_F16, "i8": b2.FMT_I8}[fmt]


def pack(fmt, xs, stride, seed=5):
    """[len(xs)][stride] samples in the layout of ``fmt``; whatever a CPI does not fill (the gap between CPIs, and tuner 2
    of the .rspduo words) holds junk.  A CPI longer than the stride is cut: only its first N samples are ever read."""
    rng = np.random.default_rng(seed)
    B = len(xs)
    if fmt == "c32":
        buf = np.full((B, stride), 30000 - 30000j, dtype=np.complex64)
    elif fmt == "i16":
        buf = rng.integers(-32768, 32768, (B, stride, 4)).astype(np.int16)
    elif fmt == "f16":
        buf = rng.integers(-2048, 2049, (B, stride, 2)).astype(np.float16)
    else:
        buf = rng.integers(-128, 128, (B, stride, 2)).astype(np.int8)
    for i, x in enumerate(xs):
        m = min(len(x), stride)
        if fmt == "c32":
            buf[i, :m] = x[:m]
        else:
            buf[i, :m, 0] = x[:m].real
            buf[i, :m, 1] = x[:m].imag
            back = buf[i, :m, 0].astype(np.float64) + 1j * buf[i, :m, 1].astype(np.float64)
            assert np.array_equal(back, x[:m]), f"{fmt} does not hold these samples exactly"
    return buf


def run_dev(b2, sa, fmt, xs, stride=None, rows=None):
    """One process_dev of the CPIs ``xs`` (stride in samples; None: the lone CPI's own length) into a guarded
    [rows][nS] output.  Returns the n_cpi rows written; asserts the guard and that no other row was touched."""
    import torch
    B = len(xs)
    rows = B if rows is None else rows
    nS = sa.nSpectrum
    buf = pack(fmt, xs, len(xs[0]) if stride is None else stride)
    d_x = torch.from_numpy(buf).cuda()
    words = rows * nS * 4
    whole = torch.full((words + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    sa.process_dev(fmt_code(b2, fmt), d_x.data_ptr(), B, 0 if stride is None else stride, whole.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = whole.cpu().numpy().view(np.uint32)
    assert (w[words:] == GUARD).all(), "guard words behind the output were written"
    assert (w[B * nS * 4:words] == GUARD).all(), f"rows {B} .. {rows - 1} of the output were written"
    out = w[:B * nS * 4].view(np.complex128).reshape(B, nS)
    assert np.isfinite(out.view(np.float64)).all(), "a bin was left unwritten (two guard words read as a NaN) or is not finite"
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. every row, FMT_C32, lone CPI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [g.name for g in SC.GEOMS], ids=[f"{g.name}-c32" for g in SC.GEOMS])
def test_lone_cpi(b2, handles, name):
    g = SC.BY_NAME[name]
    sa = handles(name)
    worst = ("", 0.0)
    for cs in SC.cases(name):
        got = run_dev(b2, sa, "c32", [cs.x])[0]
        e = SC.case_err(got, cs, g)
        worst = max(worst, (cs.tag, e), key=lambda t: t[1])
        kind, _, at = cs.tag.partition("@")
        if cs.tag == "impulse@tail":
            assert not got.any(), f"{name}: samples behind N reached the spectrum"
        elif kind == "impulse":
            closed = SC.impulse(g, int(at))[1]
            assert SC.err(got, closed) <= SC.GATE, f"{name} {cs.tag}: {SC.err(got, closed):.2e} from the closed form"
        elif kind == "tone":
            assert int(np.argmax(np.abs(got))) == int(at), f"{name} {cs.tag}: peak on bin {int(np.argmax(np.abs(got)))}"
        assert e <= SC.GATE, f"{name} {cs.tag}: {e:.2e} (gate {SC.GATE:.2e})"
        if kind in ("noise", "off-comb") or cs.tag == "impulse@0":
            for dt in (np.complex64, np.complex128):
                host, freq = sa.process(cs.x.astype(dt))
                assert freq.size == 0
                assert np.array_equal(bits(host), bits(got)), f"{name} {cs.tag}: process({dt.__name__}) is not the device call"
    print(f"\n[{name}-c32] worst {worst[1]:.2e} on {worst[0]} (gate {SC.GATE:.2e})  #fig {SC.path_of(g)} c32 {worst[1]:.3e}")


# ---- 2. the fold's chunks on this device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty-chunk", "n10030", "d16"], ids=lambda n: f"{n}-c32")
def test_fold_chunks_on_this_device(b2, name):
    """The rows of test_lone_cpi that are there for their chunks have them on the device that ran it."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = SC.BY_NAME[name]
    nJ, per = SC.fold_chunks(g, cus)
    if name == "empty-chunk":
        assert nJ < (g.D + 3) // 4 and per * (nJ - 1) >= g.D, f"{cus} CUs: {nJ} chunks of {per} leave none empty at D = {g.D}"
    elif name == "n10030":
        assert nJ > 1 and 0 < g.D - per * (nJ - 1) < per, f"{cus} CUs: {nJ} chunks of {per}: the last is not ragged at D = {g.D}"
    else:
        assert (nJ, per) == (4, 4)


# ---- 3. formats ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c32_bits(b2, handles):
    """The C32 lone-CPI result of the int8-range samples of a format row: what every other format must reproduce."""
    made = {}

    def get(name):
        if name not in made:
            g = SC.BY_NAME[name]
            x = SC.noise_plus_tone(g, 11, 100)
            got = run_dev(b2, handles(name), "c32", [x])[0]
            e = SC.err(got, SC.reference(x, g))
            assert e <= SC.GATE, f"{name}-c32 int8-range samples: {e:.2e}"
            made[name] = (x, got)
        return made[name]

    return get


@pytest.mark.parametrize("fmt", FORMATS[1:])
@pytest.mark.parametrize("name", FORMAT_ROWS)
def test_formats_same_bits(b2, handles, c32_bits, name, fmt):
    x, want = c32_bits(name)
    got = run_dev(b2, handles(name), fmt, [x])[0]
    assert np.array_equal(bits(got), bits(want)), \
        f"{name}-{fmt}: {SC.err(got, want):.2e} from the C32 call on the same samples (worst bin {int(np.argmax(np.abs(got - want)))})"


@pytest.mark.parametrize("name", FORMAT_ROWS, ids=[f"{n}-i16" for n in FORMAT_ROWS])
def test_i16_full_range(b2, handles, name):
    g = SC.BY_NAME[name]
    x = SC.noise_plus_tone(g, 12, 32767).copy()
    x[0], x[g.N - 1] = 32767 - 32768j, -32768 + 32767j
    got = run_dev(b2, handles(name), "i16", [x])[0]
    e = SC.err(got, SC.reference(x, g))
    print(f"\n[{name}-i16] {e:.2e}  #fig {SC.path_of(g)} i16 {e:.3e}")
    assert e <= SC.GATE


@pytest.mark.parametrize("name", FORMAT_ROWS, ids=[f"{n}-f16" for n in FORMAT_ROWS])
def test_f16_quarter_steps(b2, handles, name):
    g = SC.BY_NAME[name]
    x = SC.quarters(g, 13)
    got = run_dev(b2, handles(name), "f16", [x])[0]
    e = SC.err(got, SC.reference(x, g))
    print(f"\n[{name}-f16] {e:.2e}  #fig {SC.path_of(g)} f16 {e:.3e}")
    assert e <= SC.GATE


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lone_rows(b2, handles):
    """Four distinct int8-range CPIs of a batch row and the lone C32 call of each on the batch handle."""
    made = {}

    def get(name):
        if name not in made:
            g = SC.BY_NAME[name]
            sa = handles(name, MAX_BATCH)
            xs = [SC.noise_plus_tone(g, 20 + i, 100) for i in range(MAX_BATCH)]
            lone = []
            for x in xs:
                got = run_dev(b2, sa, "c32", [x], rows=MAX_BATCH)[0]
                e = SC.err(got, SC.reference(x, g))
                assert e <= SC.GATE, f"{name}: lone CPI on the batch handle: {e:.2e}"
                lone.append(got)
            made[name] = (xs, lone)
        return made[name]

    return get


def strides_of(g):
    return [("N", g.N), ("N+5", g.N + GAP)] + ([("n", g.n)] if g.n > g.N else [])


BATCH_CASES = [(name, fmt, tag) for name in BATCH_ROWS for tag, _ in strides_of(SC.BY_NAME[name]) for fmt in ("c32",)] + \
              [(name, fmt, "N+5") for name in BATCH_ROWS for fmt in FORMATS[1:]]


@pytest.mark.parametrize("name,fmt,stride", BATCH_CASES, ids=[f"{n}-{f}-stride{s}" for n, f, s in BATCH_CASES])
def test_batches(b2, handles, lone_rows, name, fmt, stride):
    g = SC.BY_NAME[name]
    sa = handles(name, MAX_BATCH)
    xs, lone = lone_rows(name)
    st = dict(strides_of(g) + [("N+5", g.N + GAP)])[stride]
    for n_cpi in ((1, 3, 4) if fmt == "c32" else (3,)):
        got = run_dev(b2, sa, fmt, xs[:n_cpi], stride=st, rows=MAX_BATCH)
        for i in range(n_cpi):
            assert np.array_equal(bits(got[i]), bits(lone[i])), \
                f"{name}-{fmt} stride {stride} n_cpi {n_cpi}: CPI {i} is {SC.err(got[i], lone[i]):.2e} from its lone call"


# ---- 5. reuse -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REUSE_ROWS, ids=[f"{n}-c32" for n in REUSE_ROWS])
def test_reuse(b2, handles, name):
    import torch
    g = SC.BY_NAME[name]
    if SC.path_of(g) != "chirpz":
        assert SC.fold_chunks(g, torch.cuda.get_device_properties(0).multi_processor_count)[0] > 1
    sa = handles(name)
    t = np.arange(g.n)
    loud = SC.TAIL * (1.0 - 2 * ((t * 7 // 3) & 1)) + 1j * SC.TAIL * (1.0 - 2 * ((t * 5 // 7) & 1))
    first = run_dev(b2, sa, "c32", [loud])[0]
    assert SC.err(first, SC.reference(loud, g)) <= SC.GATE
    silent = run_dev(b2, sa, "c32", [np.zeros(g.n, dtype=np.complex128)])[0]
    assert not silent.any(), f"{name}: {np.count_nonzero(silent)} bins of an all-zero CPI are not zero after a loud one"
    again = run_dev(b2, sa, "c32", [loud])[0]
    assert np.array_equal(bits(again), bits(first))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n1293"], ids=lambda n: f"{n}-c32")
def test_refusals(b2, handles, name):
    import torch
    from blah2_amd import _lib
    g = SC.BY_NAME[name]
    sa = handles(name, MAX_BATCH)
    d_x = torch.zeros((MAX_BATCH + 1, g.n), dtype=torch.complex64, device="cuda")
    whole = torch.full((MAX_BATCH * g.nS * 4 + PAD,), int(GUARD.view(np.int32)), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def refused(code, fmt, n_cpi, stride):
        with pytest.raises(b2.Blah2HipError) as ei:
            sa.process_dev(fmt, d_x.data_ptr(), n_cpi, stride, whole.data_ptr(), st)
        assert ei.value.code == code, ei.value
        torch.cuda.synchronize()
        assert (whole.cpu().numpy().view(np.uint32) == GUARD).all(), "a refused call wrote the output"

    refused(_lib.ERR_INVALID, b2.FMT_C32, 0, g.n)
    refused(_lib.ERR_INVALID, b2.FMT_C32, MAX_BATCH + 1, g.n)
    refused(_lib.ERR_INVALID, b2.FMT_C32, 2, g.N - 1)
    refused(_lib.ERR_INVALID, 3, 1, g.n)     # FMT_I16X_C32Y: a format of the ambiguity stage, not of this one
    refused(_lib.ERR_INVALID, 99, 1, g.n)
    refused(_lib.ERR_INVALID, -1, 1, g.n)
    sa.process_dev(b2.FMT_C32, d_x.data_ptr(), 1, g.N - 1, whole.data_ptr(), st)   # one CPI: the stride is not used
    torch.cuda.synchronize()
    w = whole.cpu().numpy().view(np.uint32)
    assert not w[:g.nS * 4].view(np.float64).any() and (w[g.nS * 4:] == GUARD).all()
    for args, code in (((1000, 0.0), _lib.ERR_INVALID), ((1000, -1.0), _lib.ERR_INVALID), ((1000, float("nan")), _lib.ERR_INVALID),
                       ((1000, 2000), _lib.ERR_INVALID), ((1000, 1000.5), _lib.ERR_INVALID),
                       (((1 << 26) + 1, float((1 << 26) + 1)), _lib.ERR_UNSUPPORTED)):
        with pytest.raises(b2.Blah2HipError) as ei:
            b2.SpectrumAnalyser(*args)
        assert ei.value.code == code, (args, ei.value)
    with pytest.raises(b2.Blah2HipError) as ei:
        b2.SpectrumAnalyser(1000, 10, max_batch=0)
    assert ei.value.code == _lib.ERR_INVALID
    for dt in (np.complex64, np.complex128):
        with pytest.raises(b2.Blah2HipError) as ei:
            sa.process(np.zeros(g.N - 1, dtype=dt))
        assert ei.value.code == _lib.ERR_INVALID
    spec, _ = sa.process(np.zeros(g.N, dtype=np.complex64))     # N of the n samples are enough
    assert not spec.any()


# ---- 7. the last direct size --------------------------------------------------------------------------------------------------
def test_last_direct_size_l2_last_c32(b2, handles):
    import torch
    g = SC.BY_NAME["l2-last"]
    cs = SC.noise_case(g.name)
    sa = handles(g.name)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = run_dev(b2, sa, "c32", [cs.x])[0]
    dt = time.perf_counter() - t0
    e = SC.case_err(got, cs, g)
    print(f"\n[l2-last-c32] nS = 65536: {e:.2e} (gate {SC.GATE:.2e}), {dt:.2f} s with the upload and the read-back  #fig l2-last c32 {e:.3e} {dt:.2f}")
    assert e <= SC.GATE
