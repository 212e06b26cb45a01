"""fp64 restatement of the clutter filter with taps per block (include/blah2hip.h, blah2hip_clutter_create_ex), and the
drifting-clutter scene on which blocks pay.

Estimation: the taps of block j are what ``oracle.blah2_oracle.wiener_hopf`` computes on the block's L samples taken alone
(shift and correlations circular inside the block).  Application: one continuous convolution over the CPI-level shifted
channel xs[i] = x[(uint32(i) - uint32(delayMin)) mod N], zero in front of sample 0, with the taps of the block the output
sample lies in -- the history of block j > 0 is block j - 1.  ``blocks = 1`` is ``wiener_hopf`` itself.

No GPU is touched here."""
import numpy as np

from oracle import blah2_oracle as O


def shifted_reference(x, delay_min):
    """xs of WienerHopf.cpp:67 over the whole CPI, the reference's own uint32 arithmetic."""
    n = x.shape[0]
    i = np.arange(n, dtype=np.uint64)
    idx = ((i - np.uint64(delay_min & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)) % np.uint64(n)
    return np.asarray(x, dtype=np.complex128)[idx.astype(np.int64)]


def wiener_hopf_blocks(x, y, delay_min, delay_max, blocks):
    """-> (ok [blocks] bool, y_filtered [N], w [blocks][nBins], r [blocks][nBins], b [blocks][nBins]).

    A block whose matrix is not positive definite has ok = False, zero taps, and passes y through (the device entry
    points' contract); the other blocks are filtered."""
    x = np.asarray(x, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128)
    n = x.shape[0]
    if blocks < 1 or n % blocks:
        raise ValueError("equal blocks only")
    L, nb = n // blocks, delay_max - delay_min
    ok = np.zeros(blocks, dtype=bool)
    w = np.zeros((blocks, nb), dtype=np.complex128)
    r = np.zeros((blocks, nb), dtype=np.complex128)
    b = np.zeros((blocks, nb), dtype=np.complex128)
    for j in range(blocks):
        okj, _, wj, rj, bj = O.wiener_hopf(x[j * L:(j + 1) * L], y[j * L:(j + 1) * L], delay_min, delay_max, return_filter=True)
        ok[j], r[j], b[j] = okj, rj, bj
        if okj:
            w[j] = wj
    xs = shifted_reference(x, delay_min)
    out = y.copy()
    for j in range(blocks):
        if not ok[j]:
            continue
        lo = max(0, j * L - (nb - 1))                       # the block's samples and nBins - 1 of history (block 0: zero fill)
        conv = np.convolve(xs[lo:(j + 1) * L], w[j])        # linear: conv[m] = sum_k w[k] xs[lo + m - k], zeros in front of lo
        seg = conv[j * L - lo:(j + 1) * L - lo]
        if j > 0:
            assert j * L - lo == nb - 1                     # every kept sample has its whole history inside [lo, ...)
        out[j * L:(j + 1) * L] -= seg
    return ok, out, w, r, b


# ---- the scene: clutter whose complex gain drifts by a cycle or two per CPI ------------------------------------------------
SCENE_N, SCENE_DMIN, SCENE_DMAX, SCENE_SEED = 32768, 0, 8, 5
SCENE_TARGET = (5, 200.0, 0.02)  # lag, cycles per CPI, amplitude

_scene = {}


def drifting_scene(n=SCENE_N, seed=SCENE_SEED):
    """(x, y) complex128: reference of amplitude 300; direct path 0.8 (1 + 0.3 e^{j 2 pi 1.5 n / N}); a second echo at lag
    3 with gain 0.2 e^{j 2 pi 0.7 n / N}; a target at lag 5, 200 cycles per CPI, amplitude 0.02; noise of amplitude 3."""
    key = (n, seed)
    if key not in _scene:
        rng = np.random.default_rng(seed)
        t = np.arange(n) / n
        x = 300.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        lag = lambda d: np.concatenate([np.zeros(d, dtype=np.complex128), x[:n - d]])
        y = 0.8 * (1.0 + 0.3 * np.exp(2j * np.pi * 1.5 * t)) * x
        y = y + 0.2 * np.exp(2j * np.pi * 0.7 * t) * lag(3)
        d, cyc, amp = SCENE_TARGET
        y = y + amp * np.exp(2j * np.pi * cyc * t) * lag(d)
        y = y + 3.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x.setflags(write=False)
        y.setflags(write=False)
        _scene[key] = (x, y)
    return _scene[key]


def residual_db(y_filtered, y):
    """Power of the filtered channel against the input's, dB."""
    return 10.0 * np.log10(np.sum(np.abs(y_filtered) ** 2) / np.sum(np.abs(y) ** 2))
