"""Python mirror of the reference's hot-path classes, on top of the C ABI.

Same names, constructor arguments, getters and call order as
/root/reference/src/process/ambiguity/Ambiguity.h:34-58,
src/data/Map.h:19-112, src/data/Detection.h:13-70 and
src/process/detection/CfarDetector1D.h:46-55, so the parity tests read like
test/unit/process/ambiguity/TestAmbiguity.cpp.  All numerics run in the HIP
library; this file only marshals buffers.  (The C++ mirror that drops into
blah2.cpp lives in blah2_amd/host/.)
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import AmbDims, Blah2HipError, check


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def ula_weights(n_surv, spacing_wavelengths, angles_deg):
    """Beam weights of a uniform line array of ``n_surv`` elements ``spacing_wavelengths`` apart, one row per angle
    (degrees off broadside): the conjugate steering vectors over the element count,
    ``w[b][k] = exp(-2j pi k d sin(theta_b)) / n_surv``, complex128 ``[n_beams, n_surv]`` -- the ``w`` of
    :meth:`Ambiguity.beamform_dev`.  Pure NumPy."""
    theta = np.deg2rad(np.atleast_1d(np.asarray(angles_deg, dtype=np.float64)))
    k = np.arange(int(n_surv), dtype=np.float64)
    return np.exp(-2j * np.pi * float(spacing_wavelengths) * np.sin(theta)[:, None] * k[None, :]) / int(n_surv)


def ula_steering(n_surv, spacing_wavelengths, angles_deg):
    """Steering vectors of the same array, one row per angle: ``a[b][k] = exp(+2j pi k d sin(theta_b))``, complex128
    ``[n_beams, n_surv]`` -- ``conj(ula_weights) * n_surv``, the ``steer`` of :meth:`Ambiguity.mvdr_weights_dev`.  Pure NumPy."""
    theta = np.deg2rad(np.atleast_1d(np.asarray(angles_deg, dtype=np.float64)))
    k = np.arange(int(n_surv), dtype=np.float64)
    return np.exp(2j * np.pi * float(spacing_wavelengths) * np.sin(theta)[:, None] * k[None, :])


def _cholesky_loaded(Rf, loading):
    """``R_l = R + loading (tr R / K) I = L L^H`` for a stack ``Rf [n, K, K]`` (the lower triangle is read), written out
    column by column in the order of mvdr_weights_kernel.  Returns ``(L [n, K, K], good [n] bool)``; ``good`` is False where a
    pivot is not finite or not positive."""
    n, K = Rf.shape[0], Rf.shape[-1]
    tr = np.zeros(n)
    for i in range(K):
        tr = tr + Rf[:, i, i].real
    delta = float(loading) * (tr / K)
    L = np.zeros((n, K, K), dtype=np.complex128)
    good = np.ones(n, dtype=bool)
    for j in range(K):
        d = Rf[:, j, j].real + delta
        for p in range(j):
            d = d - (L[:, j, p].real ** 2 + L[:, j, p].imag ** 2)
        good &= (d > 0) & np.isfinite(d)
        piv = np.sqrt(d)
        L[:, j, j] = piv
        for i in range(j + 1, K):
            v = Rf[:, i, j].copy()
            for p in range(j):
                v = v - L[:, i, p] * np.conj(L[:, j, p])
            L[:, i, j] = v / piv
    return L, good


def _forward_solve(L, a):
    """``L y = a`` by forward substitution, ``L [K, K]`` lower triangular with a real diagonal, ``a [..., K]``."""
    K = L.shape[-1]
    y = np.zeros(a.shape, dtype=np.complex128)
    for i in range(K):
        v = a[..., i].copy()
        for p in range(i):
            v = v - L[i, p] * y[..., p]
        y[..., i] = v / L[i, i].real
    return y


def mvdr_weights(R, steer, loading):
    """blah2hip_amb_mvdr_weights_dev restated in fp64 NumPy.  ``R``: Hermitian ``[..., K, K]`` (the lower triangle is read),
    ``steer``: ``[n_beams, K]``.  With ``R_l = R + loading (tr R / K) I``: ``h_b = R_l^-1 a_b / (a_b^H R_l^-1 a_b)`` through
    a Cholesky factorisation, and ``w[..., b, :] = conj(h_b)`` -- the weights of ``beamform_dev`` (``M_b = sum_k w[b][k]
    M_k``), distortionless: ``w[b] @ a_b = 1``.  Where a pivot is not finite or not positive (a zero matrix, a NaN) ``ok`` is
    0 and the weights are the conventional ``conj(a_b) / (a_b^H a_b)``.  Returns ``(w [..., n_beams, K] complex128,
    ok [...] int32)``."""
    R = np.asarray(R, dtype=np.complex128)
    a = np.atleast_2d(np.asarray(steer, dtype=np.complex128))
    K = R.shape[-1]
    if R.ndim < 2 or R.shape[-2] != K or a.shape[1] != K:
        raise ValueError("R must be [..., K, K] and steer [n_beams, K]")
    if not (np.isfinite(loading) and loading >= 0):
        raise ValueError("loading must be finite and not negative")
    if (np.abs(a).sum(axis=1) == 0).any():
        raise ValueError("a steering vector is all zero")
    batch = R.shape[:-2]
    Rf = R.reshape((-1, K, K))
    n = Rf.shape[0]
    with np.errstate(all="ignore"):
        L, good = _cholesky_loaded(Rf, loading)
        w = np.empty((n, a.shape[0], K), dtype=np.complex128)
        for b in range(a.shape[0]):
            y = np.zeros((n, K), dtype=np.complex128)
            den = np.zeros(n)
            for i in range(K):  # L y = a
                v = np.full(n, a[b, i])
                for p in range(i):
                    v = v - L[:, i, p] * y[:, p]
                y[:, i] = v / L[:, i, i].real
                den = den + y[:, i].real ** 2 + y[:, i].imag ** 2
            x = np.zeros((n, K), dtype=np.complex128)
            for i in range(K - 1, -1, -1):  # L^H x = y
                v = y[:, i].copy()
                for p in range(i + 1, K):
                    v = v - np.conj(L[:, p, i]) * x[:, p]
                x[:, i] = v / L[:, i, i].real
            w[:, b, :] = np.conj(x / den[:, None])
    conventional = np.conj(a) / (np.abs(a) ** 2).sum(axis=1)[:, None]
    w[~good] = conventional
    return w.reshape(batch + (a.shape[0], K)), good.astype(np.int32).reshape(batch)


def sample_covariance(ys, s0=0, s1=None):
    """blah2hip_amb_sample_covariance_dev restated in fp64 NumPy.  ``ys``: the channels' samples ``[K, ..., n]`` (complex, or
    anything that converts to complex128 exactly); ``R[..., i, j] = sum over s0 <= n < s1 of y_i[n] conj(y_j[n])``,
    complex128 ``[..., K, K]`` (``s1`` None: to the end).  Integer-valued samples (int8 planes) give the exact integer sums."""
    y = np.asarray(ys).astype(np.complex128)[..., s0:s1]
    return np.einsum("i...n,j...n->...ij", y, np.conj(y))


def beam_samples(ys, w):
    """blah2hip_amb_beam_samples_dev restated in fp64 NumPy: ``ys [K, ..., n]``, ``w [n_beams, K]`` (one set) or
    ``[n_cpi, n_beams, K]`` with ``ys [K, n_cpi, n]`` (a set per CPI, as ``mvdr_weights`` returns it);
    ``y_b = sum_k w[b][k] y_k``, complex128 ``[n_beams, ..., n]``."""
    y = np.asarray(ys).astype(np.complex128)
    w = np.asarray(w, dtype=np.complex128)
    if w.ndim == 3:
        return np.einsum("cbk,kcn->bcn", w, y)
    return np.einsum("bk,k...n->b...n", w, y)


def uca_steering(n_surv, radius_wavelengths, angles_deg):
    """Steering vectors of a uniform circular array of ``n_surv`` elements on a circle of ``radius_wavelengths``, element k at
    the azimuth ``2 pi k / n_surv``, one row per angle (degrees of azimuth): ``a[g][k] = exp(2j pi r cos(theta_g - 2 pi k /
    n_surv))``, complex128 ``[n_grid, n_surv]`` -- a ``steer`` table for :func:`bearing` and :meth:`Ambiguity.bearing_dev`
    (rounded to complex64 and uploaded).  Pure NumPy."""
    theta = np.deg2rad(np.atleast_1d(np.asarray(angles_deg, dtype=np.float64)))
    phi = 2.0 * np.pi * np.arange(int(n_surv), dtype=np.float64) / int(n_surv)
    return np.exp(2j * np.pi * float(radius_wavelengths) * np.cos(theta[:, None] - phi[None, :]))


def bearing_powers(snap, steer, R=None, loading=0.0):
    """The scan behind :func:`bearing`: ``(P [n, G], t^H t [n], usable [n] bool, adaptive bool)`` for snapshots ``[n, K]`` of
    one CPI; rows of snapshots that are all zero or not finite are scanned as zeros and flagged not usable."""
    s = np.ascontiguousarray(np.atleast_2d(np.asarray(snap, dtype=np.complex128)))
    a = np.atleast_2d(np.asarray(steer, dtype=np.complex128))
    n, K = s.shape
    G = a.shape[0]
    if a.shape[1] != K or G < 3:
        raise ValueError("steer must be [G >= 3, K] for snapshots [n, K]")
    L, adaptive = np.eye(K, dtype=np.complex128), False
    with np.errstate(all="ignore"):
        if R is not None:
            if not (np.isfinite(loading) and loading >= 0):
                raise ValueError("loading must be finite and not negative")
            R = np.asarray(R, dtype=np.complex128)
            if R.shape != (K, K):
                raise ValueError("R must be [K, K]")
            Lc, good = _cholesky_loaded(R[None], loading)
            if good[0]:
                L, adaptive = Lc[0], True
        v = _forward_solve(L, a)
        vv = np.zeros(G)
        for k in range(K):
            vv = vv + (v[:, k].real ** 2 + v[:, k].imag ** 2)
        usable = np.isfinite(s.view(np.float64)).all(axis=1) & (s != 0).any(axis=1)
        t = _forward_solve(L, np.where(usable[:, None], s, 0))
        tt = np.zeros(n)
        for k in range(K):
            tt = tt + (t[:, k].real ** 2 + t[:, k].imag ** 2)
        num = np.abs(t @ np.conj(v).T) ** 2
        P = np.where(vv > 0, num / np.where(vv > 0, vv, 1.0), 0.0)
    return P, tt, usable, adaptive


def bearing(snap, steer, R=None, loading=0.0, wrap=False):
    """blah2hip_amb_bearing_dev restated in fp64 NumPy for the detections of ONE CPI.  ``snap``: ``[n, K]`` (or ``[K]``) array
    snapshots, ``steer``: the table ``[G, K]``, ``R``: the CPI's Hermitian ``[K, K]`` covariance (the lower triangle is read) or
    None.  With ``R_l = R + loading (tr R / K) I = L L^H`` (the Cholesky factor and substitution order of
    :func:`mvdr_weights`; ``L = I`` without ``R`` or where the factorisation fails), ``v_g = L^-1 a_g`` and ``t = L^-1 s``:
    ``P(g) = |v_g^H t|^2 / (v_g^H v_g)`` (0 where the denominator is 0), ``index`` the first largest ``P``, ``offset`` the
    vertex of the parabola through the linear powers at ``index - 1, index, index + 1`` (0 where it does not open downwards,
    and at an end of the grid unless ``wrap`` closes it), ``power = P(index)``, ``coherence = power / (t^H t)``.  A snapshot
    that is all zero or not finite has index -1 and zeros elsewhere.  Returns ``(index int32, offset, power, coherence,
    adaptive int32)``, arrays ``[n]`` (scalars for a ``[K]`` snapshot)."""
    single = np.ndim(snap) == 1
    P, tt, ok, good = bearing_powers(snap, steer, R, loading)
    n, G = P.shape
    with np.errstate(all="ignore"):
        idx = np.argmax(P, axis=1)                            # the first of equal maxima
        rows = np.arange(n)
        p0 = P[rows, idx]
        pm, pp = P[rows, (idx - 1) % G], P[rows, (idx + 1) % G]
        den = (pm - 2.0 * p0) + pp
        inner = (idx > 0) & (idx < G - 1)
        use = (inner | bool(wrap)) & (den < 0)
        offset = np.where(use, 0.5 * (pm - pp) / np.where(use, den, 1.0), 0.0)
        coherence = np.where(tt > 0, p0 / np.where(tt > 0, tt, 1.0), 0.0)
    index = np.where(ok, idx, -1).astype(np.int32)
    offset, power, coherence = (np.where(ok, x, 0.0) for x in (offset, p0, coherence))
    adaptive = np.where(ok, 1 if good else 0, 0).astype(np.int32)
    if single:
        return int(index[0]), float(offset[0]), float(power[0]), float(coherence[0]), int(adaptive[0])
    return index, offset, power, coherence, adaptive


def bearing_degrees(index, offset, angles_deg, wrap=False):
    """``index + offset`` of :func:`bearing` / ``bearing_dev`` as an angle on the uniformly spaced grid ``angles_deg``:
    ``angles_deg[0] + (index + offset) * step``, modulo 360 when ``wrap`` is set; NaN where index is -1."""
    ang = np.asarray(angles_deg, dtype=np.float64)
    step = ang[1] - ang[0]
    index = np.asarray(index)
    deg = ang[0] + (index.astype(np.float64) + np.asarray(offset, dtype=np.float64)) * step
    if wrap:
        deg = np.mod(deg, 360.0)
    deg = np.where(index < 0, np.nan, deg)
    return deg if deg.ndim else float(deg)


def cfar_pfa(alpha, n, looks=1):
    """The false-alarm probability of the threshold ``alpha * (tot / n)`` over ``n`` training cells when every cell is the
    sum of ``looks`` looks of noise (the cell under test Gamma(L), the training sum Gamma(nL)): with ``t = alpha / n`` and
    ``m = n L``, ``sum_{k<L} C(m+k-1, k) t^k / (1+t)^(m+k)``, term by term in the log domain as blah2hip_cfar_alpha
    evaluates it.  Pure Python."""
    import math
    L, m, t = int(looks), int(n) * int(looks), float(alpha) / int(n)
    lt, l1 = math.log(t), math.log1p(t)
    lg = -m * l1
    s = math.exp(lg)
    for k in range(1, L):
        lg += math.log((m + k - 1) / k) + lt - l1
        s += math.exp(lg)
    return s


def cfar_alpha(pfa, looks=1, max_n=1):
    """blah2hip_cfar_alpha restated in pure Python: the detectors' threshold factors ``alpha[n]``, ``n = 1 .. max_n``
    (``alpha[0]`` is NaN), for cells that are sums of ``looks`` looks.  One look: ``n (pfa^(-1/n) - 1)``.  More:
    ``cfar_pfa(alpha, n, looks) = pfa`` by bisection until the interval no longer splits (its upper end).  float64
    ``[max_n + 1]``."""
    import math
    pfa, L = float(pfa), int(looks)
    if not 1 <= L <= _lib.MAX_CFAR_LOOKS:
        raise ValueError("looks outside [1, MAX_CFAR_LOOKS]")
    out = np.full(int(max_n) + 1, np.nan)
    if L == 1:
        for n in range(1, int(max_n) + 1):
            out[n] = n * (math.pow(pfa, -1.0 / n) - 1)
        return out
    if not 0.0 < pfa < 1.0:
        raise ValueError("pfa outside (0, 1) with more than one look")
    for n in range(1, int(max_n) + 1):
        lo, hi = 0.0, 1.0
        while cfar_pfa(n * hi, n, L) > pfa:
            hi *= 2.0
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if cfar_pfa(n * mid, n, L) > pfa:
                lo = mid
            else:
                hi = mid
        out[n] = n * hi
    return out


def cfar_alpha_table(pfa, looks, max_n):
    """blah2hip_cfar_alpha itself (host arithmetic of the library, no GPU touched): float64 ``[max_n + 1]``."""
    out = np.empty(int(max_n) + 1, dtype=np.float64)
    check(_lib.load().blah2hip_cfar_alpha(float(pfa), int(looks), int(max_n), _ptr(out)))
    return out


def oscfar_rank(n, rank_permille=750):
    """``k(n) = max(1, ceil(n * rank_permille / 1000))`` in integer arithmetic: which of ``n`` training cells, counted from
    the smallest, the ordered-statistic detectors take."""
    if not 1 <= int(rank_permille) <= 1000:
        raise ValueError("rank_permille outside [1, 1000]")
    return max(1, (int(n) * int(rank_permille) + 999) // 1000)


_OS_COARSE, _OS_FINE, _OS_CUT = 4096, 16384, 60.0


def _os_logfact(L):
    lf = np.zeros(L + 1)
    for j in range(2, L + 1):
        lf[j] = lf[j - 1] + np.log(float(j))
    return lf


def _os_q(t, L, lf):
    """``Q_L(t) = e^-t sum_{j<L} t^j / j!`` for an array ``t >= 0``, term by term in the log domain."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        lt = np.log(t)
        s = np.exp(-t)
        for j in range(1, L):
            s = s + np.exp(-t + j * lt - lf[j])
    return s


def _os_logdens(x, n, k, L, lf):
    """log of the density of the k-th smallest of n Gamma(L) variables, without its constant."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        lx = np.log(x)
        small = x < L
        r = np.ones_like(x)
        s = np.ones_like(x)
        for m in range(1, 100000):  # P_L(x) from its own series where x < L: no cancellation
            r = np.where(small, r * x / (L + m), 0.0)
            s = s + r
            if not (r >= 1e-17 * s).any():
                break
        Ps = np.where(x > 0, np.exp(-x + L * lx - lf[L]) * s, 0.0)
        Qq = _os_q(x, L, lf)
        P = np.where(small, Ps, 1.0 - Qq)
        Q = np.where(small, 1.0 - Ps, Qq)
        g = -x - lf[L - 1]
        if L > 1:
            g = g + (L - 1) * lx
        if k > 1:
            g = g + (k - 1) * np.log(P)
        if n > k:
            g = g + (n - k) * np.log(Q)
    return g


def _os_nodes(n, k, L, lf, alpha0=0.0):
    """Simpson nodes ``x`` and weights times density ``w`` of blah2hip_oscfar_alpha's quadrature for (n, k, L) at factors
    ``>= alpha0`` (os_nodes in csrc/cfar_alpha.hpp)."""
    logc = 0.0
    for i in range(k):
        logc += np.log(float(n - i))
    for i in range(2, k):
        logc -= np.log(float(i))

    def G(x):
        g = _os_logdens(x, n, k, L, lf)
        if alpha0 > 0.0:
            with np.errstate(all="ignore"):
                g = g + np.log(_os_q(alpha0 * x, L, lf))
        return g
    a, b = 0.0, L + 40.0 * np.sqrt(float(L)) + 100.0
    for _ in range(2):
        hc = (b - a) / _OS_COARSE
        g = G(a + hc * np.arange(_OS_COARSE + 1))
        imax = int(np.nanargmax(g))
        ilo = ihi = imax
        while ilo > 0 and not g[ilo] < g[imax] - _OS_CUT:
            ilo -= 1
        while ihi < _OS_COARSE and not g[ihi] < g[imax] - _OS_CUT:
            ihi += 1
        a, b = a + hc * ilo, a + hc * ihi
    h = (b - a) / _OS_FINE
    i = np.arange(_OS_FINE + 1)
    x = a + h * i
    simpson = np.where(i % 2 == 1, 4.0, 2.0)
    simpson[0] = simpson[-1] = 1.0
    with np.errstate(all="ignore"):
        w = simpson * (h / 3.0) * np.exp(logc + _os_logdens(x, n, k, L, lf))
    return x, w


def oscfar_pfa(alpha, n, k, looks=1, quadrature=False):
    """The false-alarm probability of the ordered-statistic threshold ``alpha * x_(k)``, the k-th smallest of ``n`` training
    cells, when every cell is the sum of ``looks`` looks of noise.  One look: ``prod_{i<k} (n - i) / (n - i + alpha)``,
    evaluated as blah2hip_oscfar_alpha does, through ``-sum log1p(alpha / (n - i))``.  More looks (or ``quadrature=True``):
    ``int f_(k)(x) Q_L(alpha x) dx`` by the library's composite Simpson rule (include/blah2hip.h).  NumPy on the host."""
    import math
    n, k, L = int(n), int(k), int(looks)
    if not 1 <= k <= n:
        raise ValueError("k outside [1, n]")
    if L == 1 and not quadrature:
        s = 0.0
        for i in range(k):
            s -= math.log1p(float(alpha) / (n - i))
        return math.exp(s)
    lf = _os_logfact(L)
    x, w = _os_nodes(n, k, L, lf, float(alpha))
    return float(np.sum(w * _os_q(float(alpha) * x, L, lf)))


def oscfar_alpha(pfa, looks=1, rank_permille=750, max_n=1, quadrature=False):
    """blah2hip_oscfar_alpha restated with NumPy on the host: ``(alpha float64 [max_n + 1], rank uint32 [max_n + 1])`` with
    ``alpha[0]`` NaN, ``rank[n] = oscfar_rank(n, rank_permille)`` and ``oscfar_pfa(alpha[n], n, rank[n], looks) = pfa`` by
    bisection until the interval no longer splits (its upper end).  ``quadrature=True`` takes one look through the
    quadrature of the other looks as well."""
    import math
    pfa, L = float(pfa), int(looks)
    if not 1 <= L <= _lib.MAX_CFAR_LOOKS:
        raise ValueError("looks outside [1, MAX_CFAR_LOOKS]")
    if not 0.0 < pfa < 1.0:
        raise ValueError("pfa outside (0, 1)")
    alpha = np.full(int(max_n) + 1, np.nan)
    rank = np.zeros(int(max_n) + 1, dtype=np.uint32)
    lf = _os_logfact(L)
    lp = math.log(pfa)
    for n in range(1, int(max_n) + 1):
        k = rank[n] = oscfar_rank(n, rank_permille)
        k = int(k)
        if L == 1 and not quadrature:
            def above(a):
                s = 0.0
                for i in range(k):
                    s -= math.log1p(a / (n - i))
                return s > lp
            lo, hi = 0.0, 1.0
            while above(hi):
                hi *= 2.0
        else:
            def above_at(a, nodes):
                return float(np.sum(nodes[1] * _os_q(a * nodes[0], L, lf))) > pfa
            lo, hi = 0.0, 1.0
            while above_at(hi, _os_nodes(n, k, L, lf, hi)) and hi <= 1e300:  # each trial on nodes of its own
                lo = hi
                hi *= 2.0
            nodes = _os_nodes(n, k, L, lf, lo)

            def above(a):
                return above_at(a, nodes)
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if above(mid):
                lo = mid
            else:
                hi = mid
        alpha[n] = hi
    return alpha, rank


def oscfar_alpha_table(pfa, looks, rank_permille, max_n):
    """blah2hip_oscfar_alpha itself (host arithmetic of the library, no GPU touched): ``(alpha float64 [max_n + 1], rank
    uint32 [max_n + 1])``."""
    alpha = np.empty(int(max_n) + 1, dtype=np.float64)
    rank = np.empty(int(max_n) + 1, dtype=np.uint32)
    check(_lib.load().blah2hip_oscfar_alpha(float(pfa), int(looks), int(rank_permille), int(max_n), _ptr(alpha), _ptr(rank)))
    return alpha, rank


def oscfar_window(window):
    """``(nGd, nTd, nGf, nTf)`` of a 1-D ``(nGuard, nTrain)`` or a 2-D window."""
    w = tuple(int(v) for v in window)
    if len(w) == 2:
        w = (w[0], w[1], 0, 0)
    if len(w) != 4 or min(w) < 0:
        raise ValueError("window: (nGuard, nTrain) or (nGuardDelay, nTrainDelay, nGuardDoppler, nTrainDoppler)")
    return w


def oscfar_hits(map, delay, doppler, noise_power, alpha, rank, window, min_delay=-128, min_doppler=0.0):
    """The ordered-statistic detectors' rule restated in fp64 NumPy for one map ``[nD, nC]`` with its axes, taking the
    tables ``alpha`` and ``rank`` as arguments (``oscfar_alpha_table`` or ``oscfar_alpha`` for the window's cell count):
    with ``p = re^2 + im^2`` and the in-bounds training cells of a cell (the window's rectangle minus its guard box, never
    delay column 0), ``hit <=> n >= 1 and #{alpha[n] * p_i < p_c} >= rank[n]``, on the cells with ``delay >= min_delay`` in
    the rows that do not have ``|doppler| < min_doppler``.  ``window``: ``(nGuard, nTrain)`` or the 2-D
    ``(nGd, nTd, nGf, nTf)``.  Returns ``(row, col, snr)`` in row-major order, ``snr = 5 log10(p) - noise_power``."""
    gd, td, gf, tf = oscfar_window(window)
    hC, hR = gd + td, gf + tf
    m = np.asarray(map)
    re, im = m.real.astype(np.float64), m.imag.astype(np.float64)
    p = re * re + im * im
    nD, nC = p.shape
    alpha = np.asarray(alpha, dtype=np.float64)
    rank = np.asarray(rank).astype(np.int64)
    T = np.full((nD + 2 * hR, nC + 2 * hC), np.inf)  # a cell that does not train is never below
    T[hR:hR + nD, hC + 1:hC + nC] = p[:, 1:]
    V = np.zeros(T.shape, dtype=bool)
    V[hR:hR + nD, hC + 1:hC + nC] = True
    offsets = [(dr, dc) for dr in range(-hR, hR + 1) for dc in range(-hC, hC + 1) if not (abs(dr) <= gf and abs(dc) <= gd)]
    n = np.zeros((nD, nC), dtype=np.int64)
    for dr, dc in offsets:
        n += V[hR + dr:hR + dr + nD, hC + dc:hC + dc + nC]
    if n.max(initial=0) >= alpha.size or n.max(initial=0) >= rank.size:
        raise ValueError("the tables are shorter than the window's cell count")
    an = alpha[n]
    below = np.zeros((nD, nC), dtype=np.int64)
    with np.errstate(all="ignore"):
        for dr, dc in offsets:
            below += an * T[hR + dr:hR + dr + nD, hC + dc:hC + dc + nC] < p
        tested = ~(np.abs(np.asarray(doppler, dtype=np.float64)) < float(min_doppler))[:, None] \
            & (np.asarray(delay) >= int(min_delay))[None, :]
        hit = tested & (n >= 1) & (below >= rank[n])
        row, col = np.nonzero(hit)
        snr = 5.0 * np.log10(p[row, col]) - float(noise_power)
    return row.astype(np.int32), col.astype(np.int32), snr


def gocfar_kind(kind):
    """``"go"`` / ``"so"`` (or the library's 1 / 2) as the library's number: BLAH2HIP_CFAR_GO, BLAH2HIP_CFAR_SO."""
    k = {"go": _lib.CFAR_GO, "so": _lib.CFAR_SO}.get(kind.lower()) if isinstance(kind, str) else kind
    if isinstance(k, bool) or k not in (_lib.CFAR_GO, _lib.CFAR_SO):
        raise ValueError(f"kind {kind!r}: 'go' or 'so'")
    return int(k)


def _goso_t(alpha, a, b):
    """``E[exp(-alpha U); U < V]`` for ``U = Gamma(a) / a``, ``V = Gamma(b) / b``: ``sum_{j<b} C(a-1+j, j) (b/a)^j s^-(a+j)``
    with ``s = 1 + (alpha + b) / a``, term by term in the log domain with the library's operations."""
    import math
    da, db = float(a), float(b)
    ls = math.log(1.0 + (alpha + db) / da)
    lr = math.log(db / da) - ls
    lg = -da * ls
    s = math.exp(lg)
    for j in range(1, b):
        lg += math.log((da - 1.0 + float(j)) / float(j)) + lr
        s += math.exp(lg)
    return s


def _goso_tail(alpha, a, b):
    """``E[exp(-alpha U); U > V]``: the series of :func:`_goso_t` from ``j = b`` on (the whole series sums to
    ``(1 + alpha/a)^-a``), positive falling terms until what is left is below 1e-17 of the sum; the library's operations."""
    import math
    da, db = float(a), float(b)
    sv = 1.0 + (alpha + db) / da
    ls = math.log(sv)
    lr = math.log(db / da) - ls
    q = (db / da) / sv
    lg = -da * ls
    for j in range(1, b + 1):
        lg += math.log((da - 1.0 + float(j)) / float(j)) + lr
    s = math.exp(lg)
    for j in range(b + 1, b + 100000000):
        f = (da - 1.0 + float(j)) / float(j)
        lg += math.log(f) + lr
        t, r = math.exp(lg), f * q
        s += t
        if not t * r > (1.0 - r) * 1e-17 * s:
            break
    return s


def gocfar_pfa(alpha, kind, a, b):
    """The false-alarm probability of the greatest-of / smallest-of rule with factor ``alpha`` over halves of ``a >= 1``
    and ``b >= 1`` training cells of one-look noise (include/blah2hip.h): smallest-of ``T(a, b) + T(b, a)``, greatest-of
    ``(1 + alpha/a)^-a + (1 + alpha/b)^-b`` minus that, summed as the tails of the two series (no cancellation).  Pure
    Python, the library's order of operations."""
    kind, a, b, alpha = gocfar_kind(kind), int(a), int(b), float(alpha)
    if a < 1 or b < 1:
        raise ValueError("a and b: at least one cell each")
    if a > b:
        a, b = b, a
    if kind == _lib.CFAR_SO:
        return _goso_t(alpha, a, b) + _goso_t(alpha, b, a)
    return _goso_tail(alpha, a, b) + _goso_tail(alpha, b, a)


def gocfar_alpha(pfa, kind, a, b):
    """blah2hip_gocfar_alpha restated in pure Python for one pair: ``gocfar_pfa(alpha, kind, a, b) = pfa`` by bisection
    until the interval no longer splits (its upper end); with one half empty the cell-averaging factor of the other,
    ``n (pfa^(-1/n) - 1)``; NaN for ``(0, 0)``."""
    import math
    pfa, kind, a, b = float(pfa), gocfar_kind(kind), int(a), int(b)
    if not 0.0 < pfa < 1.0:
        raise ValueError("pfa outside (0, 1)")
    if a < 0 or b < 0:
        raise ValueError("a and b: not negative")
    if a == 0 and b == 0:
        return math.nan
    if a == 0 or b == 0:
        n = a + b
        return n * (math.pow(pfa, -1.0 / n) - 1)
    lo, hi = 0.0, 1.0
    while gocfar_pfa(hi, kind, a, b) > pfa:
        hi *= 2.0
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return hi
        if gocfar_pfa(mid, kind, a, b) > pfa:
            lo = mid
        else:
            hi = mid


def gocfar_alpha_table(pfa, kind, a, b):
    """blah2hip_gocfar_alpha itself (host arithmetic of the library, no GPU touched) for the pairs ``(a[i], b[i])``:
    float64 ``[len(a)]``."""
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.uint32)
    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.uint32)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("a and b: two lists of one length")
    out = np.empty(a.size, dtype=np.float64)
    check(_lib.load().blah2hip_gocfar_alpha(float(pfa), gocfar_kind(kind), a.size, _ptr(a), _ptr(b), _ptr(out)))
    return out


def gocfar_window(window):
    """``(nGuard, nTrain, nRowsDoppler)`` of a 1-D ``(nGuard, nTrain)`` or a 2-D window."""
    w = tuple(int(v) for v in window)
    if len(w) == 2:
        w = (w[0], w[1], 0)
    if len(w) != 3 or min(w) < 0:
        raise ValueError("window: (nGuard, nTrain) or (nGuardDelay, nTrainDelay, nRowsDoppler)")
    return w


def gocfar_counts(n_doppler, n_delay, window):
    """``(a, b)`` int64 ``[nD, nC]``: the cells of the leading and the lagging half of every cell's window (in-bounds cells,
    never delay column 0 in the leading half)."""
    g, t, hR = gocfar_window(window)
    i, j = np.arange(int(n_doppler)), np.arange(int(n_delay))
    rows = np.minimum(i + hR, n_doppler - 1) - np.maximum(i - hR, 0) + 1
    lead = np.maximum(np.minimum(j - g, n_delay) - np.maximum(j - g - t, 1), 0)
    lag = np.maximum(np.minimum(j + g + t + 1, n_delay) - np.minimum(j + g + 1, n_delay), 0)
    return rows[:, None] * lead[None, :], rows[:, None] * lag[None, :]


def gocfar_hits(map, delay, doppler, noise_power, alpha, kind, window, min_delay=-128, min_doppler=0.0):
    """The greatest-of / smallest-of detectors' rule restated in fp64 NumPy for one map ``[nD, nC]`` with its axes
    (include/blah2hip.h).  ``p = re^2 + im^2``; the halves of cell ``(i, j)`` are the columns ``j - nG - nT .. j - nG - 1``
    (never column 0) and ``j + nG + 1 .. j + nG + nT`` inside the map, over the rows ``i - hR .. i + hR`` inside it; per
    column the rows are added in ascending order from 0.0, then the columns in ascending order from 0.0.  Both halves
    occupied: ``p_c > alpha mu_A`` and (greatest-of) / or (smallest-of) ``p_c > alpha mu_B``; one empty: the averaging
    rule over the other with the factor ``alpha`` gives for ``(a, 0)``; both: no hit.  ``alpha``: a callable
    ``alpha(a, b)`` or a dictionary over ``(a, b)``.  ``window``: ``(nGuard, nTrain)`` or ``(nGuardDelay, nTrainDelay,
    nRowsDoppler)``.  Returns ``(row, col, snr)`` in row-major order, ``snr = 5 log10(p) - noise_power``."""
    kind = gocfar_kind(kind)
    g, t, hR = gocfar_window(window)
    hC = g + t
    m = np.asarray(map)
    re, im = m.real.astype(np.float64), m.imag.astype(np.float64)
    p = re * re + im * im
    nD, nC = p.shape
    a, b = gocfar_counts(nD, nC, (g, t, hR))
    P = np.zeros((nD + 2 * hR, nC + 2 * hC))  # a cell that does not train adds an exact 0.0
    P[hR:hR + nD, hC + 1:hC + nC] = p[:, 1:]
    with np.errstate(all="ignore"):
        Csum = np.zeros((nD, nC + 2 * hC))
        for r in range(2 * hR + 1):
            Csum = Csum + P[r:r + nD]
        SA, SB = np.zeros((nD, nC)), np.zeros((nD, nC))
        for c in range(t):
            SA = SA + Csum[:, c:c + nC]
        for c in range(t):
            SB = SB + Csum[:, hC + g + 1 + c:hC + g + 1 + c + nC]
        pairs = np.unique(np.stack([a.ravel(), b.ravel()], axis=1), axis=0)
        al = np.full((nD, nC), np.nan)
        for x, y in pairs.tolist():
            if x or y:
                v = alpha(x, y) if callable(alpha) else alpha[(x, y)]
                al[(a == x) & (b == y)] = float(v)
        one = (a == 0) != (b == 0)
        both = (a > 0) & (b > 0)
        hitA = p > al * (SA / a.astype(np.float64))
        hitB = p > al * (SB / b.astype(np.float64))
        single = p > al * (np.where(a > 0, SA, SB) / (a + b).astype(np.float64))
        two = (hitA & hitB) if kind == _lib.CFAR_GO else (hitA | hitB)
        tested = ~(np.abs(np.asarray(doppler, dtype=np.float64)) < float(min_doppler))[:, None] \
            & (np.asarray(delay) >= int(min_delay))[None, :]
        hit = tested & ((both & two) | (one & single))
        row, col = np.nonzero(hit)
        snr = 5.0 * np.log10(p[row, col]) - float(noise_power)
    return row.astype(np.int32), col.astype(np.int32), snr


def gocfar_table_for(pfa, kind, n_doppler, n_delay, window):
    """The library's factors (:func:`gocfar_alpha_table`) for every pair a map of this shape gives under ``window``, as the
    dictionary :func:`gocfar_hits` takes."""
    a, b = gocfar_counts(n_doppler, n_delay, window)
    pairs = np.unique(np.stack([a.ravel(), b.ravel()], axis=1), axis=0)
    al = gocfar_alpha_table(pfa, kind, pairs[:, 0], pairs[:, 1])
    return {(int(x), int(y)): float(v) for (x, y), v in zip(pairs.tolist(), al)}


def clutter_map_weights(age, memory):
    """The weights ``c_i`` of the clutter map's average ``b = sum_i c_i u_i`` at age ``age >= 1`` (the CPIs absorbed) with
    memory ``T``, newest value first: ``age`` times ``1 / age`` while ``age <= T``; beyond, ``w (1 - w)^m`` for
    ``m = 0 .. age - T - 1`` and ``T`` times ``(1 - w)^(age - T) / T``, ``w = 1 / T`` (the powers by repeated
    multiplication, as blah2hip_cmap_alpha forms them).  float64 ``[age]``; they add up to 1."""
    a, T = int(age), int(memory)
    if a < 1 or not 1 <= T <= _lib.MAX_CMAP_MEMORY:
        raise ValueError("age below 1 or memory outside [1, MAX_CMAP_MEMORY]")
    if a <= T:
        return np.full(a, 1.0 / a)
    w = 1.0 / T
    q = 1.0 - w
    out, g = [], 1.0
    for _ in range(a - T):
        out.append(w * g)
        g *= q
    return np.array(out + [g / T] * T)


def _cmap_logpfa(alpha, a, T):
    """cmap_logpfa of cfar_alpha.hpp, operation for operation (libm's log1p, the sum in the same order)."""
    import math
    w = 1.0 / T
    q = 1.0 - w
    g, s = 1.0, 0.0
    for _ in range(a - T):
        s -= math.log1p(alpha * (w * g))
        g *= q
    return s - T * math.log1p(alpha * (g / T))


def clutter_map_pfa(alpha, age, memory):
    """The false-alarm probability of ``u > alpha b`` under noise at age ``age`` with memory ``memory``:
    ``prod_i 1 / (1 + alpha c_i)`` over :func:`clutter_map_weights`, through the sum of ``log1p``."""
    import math
    a, T = int(age), int(memory)
    if a <= T:
        return math.exp(-a * math.log1p(float(alpha) / a))
    return math.exp(_cmap_logpfa(float(alpha), a, T))


def clutter_map_alpha(pfa, memory, max_age):
    """blah2hip_cmap_alpha restated in pure Python: the clutter map's threshold factors ``alpha[a]``, ``a = 1 .. max_age``
    (``alpha[0]`` is NaN).  ``a <= T``: ``a (pfa^(-1/a) - 1)``.  Beyond: ``clutter_map_pfa(alpha, a, T) = pfa`` by bisection on
    its logarithm until the interval no longer splits (its upper end); entries beyond ``16 T`` repeat that one.  float64
    ``[max_age + 1]``."""
    import math
    pfa, T, n = float(pfa), int(memory), int(max_age)
    if not 1 <= T <= _lib.MAX_CMAP_MEMORY:
        raise ValueError("memory outside [1, MAX_CMAP_MEMORY]")
    if not 0.0 < pfa < 1.0:
        raise ValueError("pfa outside (0, 1)")
    out = np.full(n + 1, np.nan)
    last = min(n, 16 * T)
    lp = math.log(pfa)
    for a in range(1, last + 1):
        if a <= T:
            out[a] = a * (math.pow(pfa, -1.0 / a) - 1)
            continue
        lo, hi = 0.0, 1.0
        while _cmap_logpfa(hi, a, T) > lp:
            hi *= 2.0
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if _cmap_logpfa(mid, a, T) > lp:
                lo = mid
            else:
                hi = mid
        out[a] = hi
    out[last + 1:] = out[last]
    return out


def clutter_map_alpha_table(pfa, memory, max_age):
    """blah2hip_cmap_alpha itself (host arithmetic of the library, no GPU touched): float64 ``[max_age + 1]``."""
    out = np.empty(int(max_age) + 1, dtype=np.float64)
    check(_lib.load().blah2hip_cmap_alpha(float(pfa), int(memory), int(max_age), _ptr(out)))
    return out


def clutter_map(maps, levels, alpha, memory, state=None, detail=False):
    """The clutter-map detector of include/blah2hip.h restated in fp64 NumPy.  ``maps``: complex ``[n_cpi, n_doppler,
    n_delay]`` in time order; ``levels``: ``[n_cpi]`` factors ``s[c]`` (the device's ``d_out_level``, or ``10 ** (-noisePower /
    5)``), None for the detector without normalisation; ``alpha``: the table of :func:`clutter_map_alpha` for at least
    ``min(last age, 16 T)`` entries; ``state``: the dict an earlier call returned through this argument (``{"b", "age",
    "umax"}``; None or empty: age 0).  Per CPI ``u = |M|^2 s``, ``exceeds <=> age >= 1 and u > alpha[min(age, 16 T)] b``,
    then ``b = u`` at age 0 and ``b += r (u - b)`` with ``r`` the fp32 quotient ``1 / min(age + 1, T)`` otherwise; a cell
    whose ``u`` is not finite neither exceeds nor updates (at age 0 it starts from ``b = 0``).  Returns ``(exceed uint8
    [n_cpi, n_doppler, n_delay], b float64 [n_doppler, n_delay])`` and updates ``state`` (``umax``: the largest ``u`` a cell
    has absorbed).  ``detail``: a third value ``{"u", "thr"}``, both ``[n_cpi, ...]``: ``u`` and ``alpha b`` at the decision
    (``thr`` is NaN at age 0)."""
    m = np.asarray(maps)
    if m.ndim != 3:
        raise ValueError("maps must be [n_cpi, n_doppler, n_delay]")
    T = int(memory)
    if not 1 <= T <= _lib.MAX_CMAP_MEMORY:
        raise ValueError("memory outside [1, MAX_CMAP_MEMORY]")
    alpha = np.asarray(alpha, dtype=np.float64)
    state = {} if state is None else state
    age = int(state.get("age", 0))
    b = np.zeros(m.shape[1:]) if age == 0 else np.array(state["b"], dtype=np.float64)
    umax = np.zeros(m.shape[1:]) if age == 0 else np.array(state["umax"], dtype=np.float64)
    exceed = np.zeros(m.shape, dtype=np.uint8)
    us, thrs = [], []
    for c in range(m.shape[0]):
        re, im = m[c].real.astype(np.float64), m[c].imag.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            u = re * re + im * im
            if levels is not None:
                u = u * float(levels[c])
            fin = np.isfinite(u)
            thr = np.full(u.shape, np.nan)
            if age >= 1:
                thr = alpha[min(age, 16 * T)] * b
                exceed[c] = fin & (u > thr)
            if age == 0:
                b = np.where(fin, u, 0.0)
            else:
                r = float(np.float32(1.0) / np.float32(min(age + 1, T)))
                b = np.where(fin, b + r * (np.where(fin, u, 0.0) - b), b)
            umax = np.where(fin, np.maximum(umax, np.where(fin, u, 0.0)), umax)
        if detail:
            us.append(u)
            thrs.append(thr)
        age += 1
    state.update(b=b, age=age, umax=umax)
    if detail:
        return exceed, b, {"u": np.array(us), "thr": np.array(thrs)}
    return exceed, b


def gate_hits(hits, count, exceed):
    """hits_gate_kernel restated: of the first ``min(count, cap)`` records of ``hits`` (:data:`HIT_DTYPE` ``[cap]``, one
    CPI) those inside the map whose byte of ``exceed [n_doppler, n_delay]`` is not zero, in their order."""
    h = np.asarray(hits)[:min(int(count), len(hits))]
    ex = np.asarray(exceed)
    inside = (h["row"] >= 0) & (h["row"] < ex.shape[0]) & (h["col"] >= 0) & (h["col"] < ex.shape[1])
    keep = inside.copy()
    keep[inside] = ex[h["row"][inside], h["col"][inside]] != 0
    return h[keep]


def integrate_ends(n_cpi, window, hop=None, start=0):
    """The CPI counts ``g`` at which a window of ``window`` CPIs ends among the CPIs ``start .. start + n_cpi - 1`` of an
    integrator with hop ``hop`` (None: 1): every ``g >= window - 1`` with ``(g - (window - 1)) % hop == 0``."""
    W, H = int(window), int(hop) if hop is not None else 1
    return [g for g in range(int(start), int(start) + int(n_cpi)) if g >= W - 1 and (g - (W - 1)) % H == 0]


def integrate_maps(maps, w=None, window=1, hop=None):
    """blah2hip_nci_process_dev restated in fp64 NumPy for a fresh integrator.  ``maps``: complex ``[K, n_cpi, nD, nC]``,
    ``w``: the ``K`` channel weights (None: all 1).  ``p[g] = sum_k w_k |M_k[g]|^2`` and, for every ``g`` of
    :func:`integrate_ends`, ``sqrt(scale (p[g-W+1] + ... + p[g]))`` with ``scale = 1 / (W sum_k w_k)`` rounded to fp32 as
    the library rounds it.  Returns float64 ``[n_out, nD, nC]``: the real parts of the output maps (the imaginary parts
    are zero)."""
    m = np.asarray(maps).astype(np.complex128)
    if m.ndim != 4:
        raise ValueError("maps must be [K, n_cpi, nD, nC]")
    K, n_cpi = m.shape[:2]
    W = int(window)
    wk = np.ones(K, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    if wk.shape != (K,):
        raise ValueError("w must hold one weight per channel")
    scale = float(np.float32(1.0 / (W * wk.astype(np.float64).sum())))
    with np.errstate(all="ignore"):
        p = np.zeros(m.shape[1:])
        for k in range(K):
            p = p + float(wk[k]) * (m[k].real ** 2 + m[k].imag ** 2)
        out = []
        for g in integrate_ends(n_cpi, W, hop):
            s = np.zeros(m.shape[2:])
            for c in range(g - W + 1, g + 1):
                s = s + p[c]
            out.append(np.sqrt(scale * s))
    return np.stack(out) if out else np.zeros((0,) + m.shape[2:])


def nci_walk_table(dims, fc, spacing=1.0):
    """``blah2hip_nci_walk_table`` restated: the physical walk between CPIs ``walk[j] = -doppler[j] * n_corr *
    n_doppler_bins * spacing / fc`` (fp64, evaluated left to right: the library's bits) in delay cells per CPI, negative for
    an approaching target.  ``spacing``: the distance between CPI starts in CPI lengths.  ``dims``: anything with
    ``doppler``, ``n_corr`` and ``n_doppler_bins`` (the oracle's ``ambiguity_dims``), or an :class:`Ambiguity`, whose
    table the library itself computes."""
    fc, spacing = float(fc), float(spacing)
    if not math.isfinite(fc) or not fc > 0.0:
        raise ValueError("the carrier frequency must be finite and positive")
    if not math.isfinite(spacing) or not spacing > 0.0:
        raise ValueError("the CPI spacing must be finite and positive")
    if isinstance(dims, Ambiguity):
        walk = np.zeros(dims.dims.n_doppler_bins, dtype=np.float64)
        check(dims._L.blah2hip_nci_walk_table(dims._h, fc, spacing, _ptr(walk)))
        return walk
    doppler = np.asarray(dims.doppler, dtype=np.float64)
    return -doppler * float(dims.n_corr) * float(dims.n_doppler_bins) * spacing / fc


def track_tables(walk, q, window):
    """The integer tables ``blah2hip_nci_set_tracks`` builds, ``(jr, s)`` as int32 ``[K, W, nD]``:
    ``r = rint(q[k] * a)``, ``jr = j - r`` (-1 where it leaves ``[0, nD)``, with ``s`` 0 there) and
    ``s = rint(-0.5 * a * (walk[j] + walk[jr]))``, in fp64 with ties to even.  ``walk``: ``[nD]``; ``q``: the bank (None:
    ``{0}``)."""
    walk = np.asarray(walk, dtype=np.float64)
    q = np.zeros(1) if q is None or np.size(q) == 0 else np.atleast_1d(np.asarray(q, dtype=np.float64))
    if walk.ndim != 1 or q.ndim != 1:
        raise ValueError("walk must be [nD] and q a bank of rates")
    if not (np.isfinite(walk).all() and np.isfinite(q).all()):
        raise ValueError("walk and q must be finite")
    nD, W = walk.size, int(window)
    j = np.arange(nD, dtype=np.int64)
    jr = np.full((q.size, W, nD), -1, dtype=np.int32)
    s = np.zeros((q.size, W, nD), dtype=np.int32)
    for k in range(q.size):
        for a in range(W):
            src = j - int(np.rint(q[k] * float(a)))
            ok = (src >= 0) & (src < nD)
            sh = np.rint(-0.5 * float(a) * (walk[j[ok]] + walk[src[ok]]))
            if sh.size and np.abs(sh).max() > _lib.MAX_TRACK_SHIFT:
                raise ValueError(f"a shift above {_lib.MAX_TRACK_SHIFT} cells")
            jr[k, a, ok] = src[ok]
            s[k, a, ok] = sh
    return jr, s


def integrate_tracks(maps, walk, q, w=None, window=1, hop=None):
    """blah2hip_nci_process_tracks_dev restated in fp64 NumPy for a fresh integrator.  ``maps``: complex
    ``[K, n_cpi, nD, nC]``; ``walk``: ``[nD]`` delay cells per CPI (None: zero); ``q``: the bank of Doppler rows per CPI
    (None: ``{0}``); ``w``, ``window``, ``hop`` as in :func:`integrate_maps`.  For every window end ``g`` of
    :func:`integrate_ends`: ``S_k[j, d] = sum_a p[g - a][jr, d + s]`` over the ages ``a = W - 1 .. 0`` with the tables of
    :func:`track_tables`, a term outside the map contributing zero.  Returns ``(levels, index, sums)``:
    ``sqrt(scale S_k*)`` float64 ``[n_out, nD, nC]``, ``k*`` uint8 (the smallest ``k`` with the largest sum; NaN sums never
    win against ``S_0``) and every ``S_k`` ``[K_bank, n_out, nD, nC]``."""
    m = np.asarray(maps).astype(np.complex128)
    if m.ndim != 4:
        raise ValueError("maps must be [K, n_cpi, nD, nC]")
    K, n_cpi, nD, nC = m.shape
    W = int(window)
    wk = np.ones(K, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    if wk.shape != (K,):
        raise ValueError("w must hold one weight per channel")
    walk = np.zeros(nD) if walk is None else np.asarray(walk, dtype=np.float64)
    if walk.shape != (nD,):
        raise ValueError("walk must hold one entry per Doppler row")
    jr, s = track_tables(walk, q, W)
    Kb = jr.shape[0]
    scale = float(np.float32(1.0 / (W * wk.astype(np.float64).sum())))
    ends = integrate_ends(n_cpi, W, hop)
    d = np.arange(nC, dtype=np.int64)
    with np.errstate(all="ignore"):
        p = np.zeros(m.shape[1:])
        for k in range(K):
            p = p + float(wk[k]) * (m[k].real ** 2 + m[k].imag ** 2)
        sums = np.zeros((Kb, len(ends), nD, nC))
        for o, g in enumerate(ends):
            for k in range(Kb):
                acc = np.zeros((nD, nC))
                for a in range(W - 1, -1, -1):
                    col = d[None, :] + s[k, a].astype(np.int64)[:, None]
                    ok = (jr[k, a] >= 0)[:, None] & (col >= 0) & (col < nC)
                    src = p[g - a][np.clip(jr[k, a], 0, nD - 1)[:, None], np.clip(col, 0, nC - 1)]
                    acc = acc + np.where(ok, src, 0.0)
                sums[k, o] = acc
        index = np.zeros((len(ends), nD, nC), dtype=np.uint8)
        best = sums[0].copy() if Kb else np.zeros((0, nD, nC))
        for k in range(1, Kb):
            win = sums[k] > best
            best = np.where(win, sums[k], best)
            index[win] = k
        levels = np.sqrt(scale * best)
    return levels, index, sums


def carrier_ratios(fc, offsets):
    """``ratio[c] = (fc + off_c) / (fc + off_0)`` for carriers at ``fc + off_c`` Hz: carrier 0 is the reference, whose
    Doppler axis the fused maps keep."""
    off = np.atleast_1d(np.asarray(offsets, dtype=np.float64))
    f = float(fc) + off
    if off.ndim != 1 or off.size < 1 or not np.all(np.isfinite(f)) or not np.all(f > 0.0):
        raise ValueError("every carrier frequency fc + offset must be finite and positive")
    return f / f[0]


def _carrier_interp(interp):
    if interp in _lib.CARRIER_INTERPS:
        return _lib.CARRIER_INTERPS[interp]
    if interp in (_lib.CARRIER_NEAREST, _lib.CARRIER_LINEAR) and not isinstance(interp, bool):
        return int(interp)
    raise ValueError(f"unknown carrier interpolation {interp!r} (nearest | linear)")


def carrier_table(doppler_axis, ratio, interp="nearest"):
    """``blah2hip_carrier_table`` restated in fp64 NumPy, its bits: for carrier ``c`` and output row ``j``
    ``u = (ratio[c] doppler[j] - doppler[0]) / D`` (left to right, ``D`` the axis' mean step), snapped to ``rint(u)`` within
    1e-9, clamped to ``[0, nD - 1]`` where the carrier does not cover the row.  ``interp``: ``"nearest"`` (``row =
    floor(u + 0.5)``, weights 1, 0) or ``"linear"`` (``row = floor(u)``, ``a_hi = fp32(u - row)``, ``a_lo = fp32(1 - (u -
    row))``).  Returns ``{"row": int32 [C, nD], "a_lo", "a_hi": float32 [C, nD], "covered": uint32 [nD]}``.  ValueError where
    the library returns BLAH2HIP_ERR_INVALID: not 1 .. 8 carriers, a ratio that is not finite or outside [0.5, 2], an
    unknown interpolation, fewer than two Doppler bins."""
    mode = _carrier_interp(interp)
    dop = np.asarray(doppler_axis, dtype=np.float64)
    r = np.atleast_1d(np.asarray(ratio, dtype=np.float64))
    if r.ndim != 1 or not 1 <= r.size <= _lib.MAX_CARRIERS:
        raise ValueError("n_carriers outside [1, 8]")
    if not np.all(np.isfinite(r)) or not np.all((r >= 0.5) & (r <= 2.0)):
        raise ValueError("a ratio is not finite or lies outside [0.5, 2]")
    if dop.ndim != 1 or dop.size < 2:
        raise ValueError("fewer than two Doppler bins")
    nD = dop.size
    top = float(nD - 1)
    delta = (dop[nD - 1] - dop[0]) / top
    u = (r[:, None] * dop[None, :] - dop[0]) / delta
    near = np.rint(u)
    u = np.where(np.abs(u - near) <= 1e-9, near, u)
    covered = ((u >= 0.0) & (u <= top)).sum(axis=0).astype(np.uint32)
    u = np.minimum(np.maximum(u, 0.0), top)
    if mode == _lib.CARRIER_NEAREST:
        row = np.floor(u + 0.5)
        a_lo, a_hi = np.ones(u.shape, dtype=np.float32), np.zeros(u.shape, dtype=np.float32)
    else:
        row = np.floor(u)
        t = u - row
        a_lo, a_hi = (1.0 - t).astype(np.float32), t.astype(np.float32)
    return {"row": row.astype(np.int32), "a_lo": a_lo, "a_hi": a_hi, "covered": covered}


def fuse_carriers(maps, table, w=None):
    """blah2hip_amb_fuse_carriers_dev restated in fp64 NumPy.  ``maps``: complex ``[C, n_cpi, nD, nC]``, ``table``:
    :func:`carrier_table`'s (or the library's own, :meth:`Ambiguity.carrier_table`) with its fp32 ``a_lo``, ``a_hi`` as
    stored, ``w``: the ``C`` carrier weights (None: all 1).  ``S = sum_c w_c (a_lo |M_c[row]|^2 + a_hi |M_c[row + 1]|^2)``,
    the second term only where ``a_hi != 0``, and ``sqrt(scale S)`` with ``scale = 1 / sum_c w_c`` rounded to fp32 as the
    library rounds it.  Returns float64 ``[n_cpi, nD, nC]``: the real parts of the output maps (the imaginary parts are
    zero)."""
    m = np.asarray(maps).astype(np.complex128)
    if m.ndim != 4:
        raise ValueError("maps must be [C, n_cpi, nD, nC]")
    C_, _, nD, _ = m.shape
    row = np.asarray(table["row"])
    a_lo, a_hi = np.asarray(table["a_lo"], dtype=np.float32), np.asarray(table["a_hi"], dtype=np.float32)
    if row.shape != (C_, nD) or a_lo.shape != (C_, nD) or a_hi.shape != (C_, nD):
        raise ValueError("the table must hold one entry per (carrier, Doppler row) of the maps")
    wc = np.ones(C_, dtype=np.float32) if w is None else np.asarray(w, dtype=np.float32)
    if wc.shape != (C_,):
        raise ValueError("w must hold one weight per carrier")
    scale = float(np.float32(1.0 / wc.astype(np.float64).sum()))
    with np.errstate(all="ignore"):
        S = np.zeros(m.shape[1:])
        for c in range(C_):
            p = m[c].real ** 2 + m[c].imag ** 2
            q = a_lo[c].astype(np.float64)[None, :, None] * p[:, row[c], :]
            hi = np.nonzero(a_hi[c] != 0)[0]  # where a_hi == 0 row + 1 is not read: a NaN there stays out
            if hi.size:
                q[:, hi, :] = q[:, hi, :] + a_hi[c, hi].astype(np.float64)[None, :, None] * p[:, row[c, hi] + 1, :]
            S = S + float(wc[c]) * q
        return np.sqrt(scale * S)


# a_0 .. a_P of the cosine-sum windows w[i] = sum_p (-1)^p a_p cos(2 pi p i / n): blah2hip_doppler_taper's table
TAPER_COEFFS = {
    "none": (1.0,),
    "hann": (0.5, 0.5),
    "hamming": (0.54, 0.46),
    "blackman": (0.42, 0.5, 0.08),
    "blackmanharris": (0.35875, 0.48829, 0.14128, 0.01168),
    "nuttall": (0.3635819, 0.4891775, 0.1365995, 0.0106411),
    "flattop": (0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368),
}


def _taper_coeffs(name):
    try:
        return TAPER_COEFFS[str(name).lower()]
    except KeyError:
        raise ValueError(f"unknown Doppler window {name!r}: one of {', '.join(TAPER_COEFFS)}") from None


def doppler_taper(name, normalise=False):
    """The taps ``t_0 .. t_P`` (fp64) of the circular Doppler stencil that equals the named slow-time window:
    ``t_0 = a_0``, ``t_m = (-1)^m a_m / 2``.  ``normalise`` divides by ``a_0``, so that an echo on a Doppler bin keeps its
    amplitude.  ``blah2hip_doppler_taper`` returns their fp32 roundings (:func:`doppler_taper_f32`)."""
    a = _taper_coeffs(name)
    t = np.array([a[0]] + [(-0.5 if m & 1 else 0.5) * a[m] for m in range(1, len(a))], dtype=np.float64)
    return t / a[0] if normalise else t


def doppler_taper_f32(name, normalise=False):
    """``blah2hip_doppler_taper``: the library's own fp32 taps of a named window, ``n_side + 1`` of them."""
    key = str(name).lower()
    _taper_coeffs(key)
    taps = np.zeros(_lib.MAX_TAPER_SIDE + 1, dtype=np.float32)
    n_side = C.c_uint32(0)
    check(_lib.load().blah2hip_doppler_taper(_lib.TAPER_KINDS[key], int(bool(normalise)), _ptr(taps), C.byref(n_side)))
    return taps[:n_side.value + 1].copy()


def doppler_window(name, n):
    """``w[i] = sum_p (-1)^p a_p cos(2 pi p i / n)``, ``i = 0 .. n - 1``: the periodic ("DFT-even") form,
    ``scipy.signal.get_window(name, n, fftbins=True)``."""
    a = _taper_coeffs(name)
    i = np.arange(int(n), dtype=np.float64)
    w = np.zeros(int(n))
    for p_, ap in enumerate(a):
        w += (-1.0) ** p_ * ap * np.cos(2.0 * np.pi * p_ * i / int(n))
    return w


def taper_maps(maps, taps):
    """blah2hip_amb_taper_dev restated in fp64 NumPy: the circular stencil along axis -2 (the Doppler rows) of ``maps``,
    ``M'[j] = t_0 M[j] + sum_m t_m (M[j - m] + M[j + m])`` with the rows taken modulo nD."""
    m = np.asarray(maps)
    m = m.astype(np.complex128 if np.iscomplexobj(m) else np.float64)
    t = np.asarray(taps, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("taps must be t_0 .. t_P")
    if m.ndim < 2 or m.shape[-2] < 2 * (t.size - 1) + 1:
        raise ValueError("fewer Doppler rows than the stencil has taps")
    with np.errstate(all="ignore"):
        out = t[0] * m
        for k in range(1, t.size):
            out = out + t[k] * np.roll(m, k, axis=-2)
            out = out + t[k] * np.roll(m, -k, axis=-2)
    return out


def taper_gains(taps):
    """What a stencil does to echoes and noise: ``(coherent_gain, noise_power_gain, enbw_bins, snr_loss_db)`` -- the
    amplitude gain ``t_0`` of an echo on a Doppler bin, the power gain ``t_0^2 + 2 sum t_m^2`` of white noise, their ratio
    ``noise / coherent^2`` (the equivalent noise bandwidth in bins) and ``10 log10`` of it (the SNR an on-bin echo loses)."""
    t = np.asarray(taps, dtype=np.float64)
    coherent = float(t[0])
    noise = float(t[0] ** 2 + 2.0 * np.sum(t[1:] ** 2))
    enbw = noise / coherent ** 2
    return coherent, noise, enbw, 10.0 * math.log10(enbw)


def migration_table(dims, fc):
    """``blah2hip_migration_table`` restated: the physical half walks ``h[j] = -0.5 * doppler[j] * n_corr / fc`` (fp64, samples
    per pulse divided by 2) of a geometry.  ``dims``: anything with ``doppler`` and ``n_corr`` (the oracle's
    ``ambiguity_dims``), or an :class:`Ambiguity`.  Positive Doppler is an approaching target: its delay decreases."""
    fc = float(fc)
    if not math.isfinite(fc) or not fc > 0.0:
        raise ValueError("the carrier frequency must be finite and positive")
    doppler = np.asarray(dims.doppler, dtype=np.float64)
    n_corr = dims.dims.n_corr if isinstance(dims, Ambiguity) else dims.n_corr
    return -0.5 * doppler * float(n_corr) / fc


def migration_shifts(half_walk, nD):
    """The shifts ``s[j, i] = rint(h[j] * (2 i - (nD - 1)))`` as int64 ``[len(h), nD]``: one fp64 multiply, ties to even --
    the bits the library works out on the device."""
    h = np.asarray(half_walk, dtype=np.float64).reshape(-1, 1)
    t = (2 * np.arange(int(nD), dtype=np.int64) - (int(nD) - 1)).astype(np.float64).reshape(1, -1)
    return np.rint(h * t).astype(np.int64)


def range_map(dims, x, y):
    """The range half of ``Ambiguity::process`` (Ambiguity.cpp:92-146) in fp64: ``R[i][d]``, pulse ``i``, delay column ``d``,
    complex128 ``[n_doppler_bins, n_delay_bins]`` -- what the Doppler transform of the map reads.  ``dims``: the oracle's
    ``ambiguity_dims``."""
    x = np.asarray(x, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128)
    nD, nC, nfft = int(dims.n_doppler_bins), int(dims.n_corr), int(dims.nfft)
    if dims.doppler_middle != 0:  # :95-102: the reference channel is rotated to the middle of the Doppler limits
        i = np.arange(x.shape[0], dtype=np.float64)
        x = x * np.exp(1j * 2.0 * np.pi * dims.doppler_middle * (i / dims.fs))
    used = nD * nC
    X = np.fft.fft(x[:used].reshape(nD, nC), n=nfft, axis=1)
    Y = np.fft.fft(y[:used].reshape(nD, nC), n=nfft, axis=1)
    Z = np.fft.ifft(Y * np.conj(X), axis=1)
    lag = (int(dims.delay_min) + np.arange(int(dims.n_delay_bins))) % nfft  # :132-146
    return Z[:, lag]


def _walk_rows(R, h):
    """The row gather of :func:`migrate_maps` and :func:`rate_bank_maps`: for every Doppler row ``j`` of the complex128
    ``R[..., nD, nDelay]``, ``(j, g, w)`` with ``g[..., i, d] = [0 <= d + s(j,i) < nDelay] R[..., i, d + s(j,i)]`` (the shifts of
    :func:`migration_shifts` for the half walks ``h``) and the row's twiddles ``w[i] = W[(i src(j)) mod nD]``,
    ``src(j) = (j + nD // 2 + 1) % nD``.  ``migrate_maps`` sums ``g w`` over the pulses: the ``q = 0`` hypothesis of the bank."""
    nD, nDelay = R.shape[-2:]
    s = migration_shifts(h, nD)
    i = np.arange(nD)
    d = np.arange(nDelay)
    for j in range(nD):
        w = np.exp(-2j * np.pi * ((i * ((j + nD // 2 + 1) % nD)) % nD) / nD)
        c = d[None, :] + s[j][:, None]  # [pulse, column]
        ok = (c >= 0) & (c < nDelay)
        yield j, np.where(ok, np.take_along_axis(R, np.broadcast_to(np.clip(c, 0, nDelay - 1), R.shape), axis=-1), 0.0), w


def migrate_maps(R, half_walk):
    """blah2hip_amb_migrate_dev restated in fp64 NumPy for EVERY row (the library copies the zero-shift rows from its input
    map instead): ``M'[j][d] = sum_i [0 <= d + s(j,i) < nDelay] R[i][d + s(j,i)] W[(i src(j)) mod nD]`` with
    ``src(j) = (j + nD // 2 + 1) % nD`` and the shifts of :func:`migration_shifts`.  ``R``: complex ``[..., nD, nDelay]``."""
    R = np.asarray(R).astype(np.complex128)
    nD = R.shape[-2]
    h = np.asarray(half_walk, dtype=np.float64)
    if h.shape != (nD,):
        raise ValueError("half_walk must hold one entry per Doppler row")
    out = np.zeros(R.shape, dtype=np.complex128)
    for j, g, w in _walk_rows(R, h):
        out[..., j, :] = np.sum(g * w[:, None], axis=-2)
    return out


def doppler_rate(dims, fc, accel):
    """``blah2hip_doppler_rate`` restated: the Doppler rate ``q = -accel * fc / 299792458 * T**2`` in bins drifted over the CPI
    of ``T = n_doppler_bins * n_corr / fs`` seconds, for the carrier ``fc`` (Hz) and the second derivative ``accel`` of the
    bistatic range (m/s^2).  ``dims``: anything with ``n_doppler_bins``, ``n_corr`` and ``fs`` (the oracle's
    ``ambiguity_dims``), or an :class:`Ambiguity`.  A receding acceleration lowers the Doppler: ``q`` is negative."""
    if isinstance(dims, Ambiguity):
        return dims.doppler_rate(fc, accel)
    fc, accel = float(fc), float(accel)
    if not math.isfinite(fc) or not fc > 0.0:
        raise ValueError("the carrier frequency must be finite and positive")
    if not math.isfinite(accel):
        raise ValueError("the acceleration must be finite")
    T = float(dims.n_doppler_bins) * float(dims.n_corr) / float(dims.fs)
    return -accel * fc / 299792458.0 * T * T


def rate_bank(q_max, step=1.0):
    """The symmetric bank ``-n step .. n step`` with ``n = floor(q_max / step)``: fp64, ascending, 0 in the middle.
    ValueError above ``BLAH2HIP_MAX_RATES`` = 16 entries (so at most 15 here), or for a ``q_max`` or ``step`` that is not
    finite, a negative ``q_max``, a ``step`` that is not positive."""
    q_max, step = float(q_max), float(step)
    if not (math.isfinite(q_max) and math.isfinite(step)) or q_max < 0.0 or not step > 0.0:
        raise ValueError("rate_bank needs a finite q_max >= 0 and a finite step > 0")
    n = int(math.floor(q_max / step * (1.0 + 1e-12)))
    if 2 * n + 1 > _lib.MAX_RATES:
        raise ValueError(f"a bank of {2 * n + 1} rates: at most {_lib.MAX_RATES}")
    return np.arange(-n, n + 1, dtype=np.float64) * step


def rate_chirps(q, nD):
    """The chirp table of ``blah2hip_amb_set_rates`` in fp64: ``c[k, i] = exp(-1j * theta_k(i))`` with
    ``theta_k(i) = pi * q[k] * t(i)**2 / (4 nD**2)``, ``t(i) = 2 i - (nD - 1)``; complex128 ``[len(q), nD]``.  The library
    rounds its real and imaginary parts to fp32."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    nD = int(nD)
    t = 2 * np.arange(nD, dtype=np.int64) - (nD - 1)
    th = np.pi * q[:, None] * (t * t).astype(np.float64)[None, :] / (4.0 * float(nD) * float(nD))
    return np.cos(th) + 1j * (-np.sin(th))


def rate_bank_maps(R, q, half_walk=None):
    """blah2hip_amb_rate_bank_dev restated in fp64 NumPy for EVERY row (the library takes a zero rate's candidate in a
    zero-shift row from its input map instead): ``M_k[j][d] = sum_i [0 <= d + s(j,i) < nDelay] R[i][d + s(j,i)] c_k[i]
    W[(i src(j)) mod nD]`` with the chirps of :func:`rate_chirps` and the shifts of :func:`migration_shifts` (``half_walk``
    None: no walk).  ``R``: complex ``[..., nD, nDelay]``.  Returns ``(maps, index, all_hypotheses)``: the strongest
    hypothesis per cell ``[..., nD, nDelay]``, its index (uint8, the smallest of equals) and every ``M_k``
    ``[K, ..., nD, nDelay]``."""
    R = np.asarray(R).astype(np.complex128)
    nD = R.shape[-2]
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not 1 <= q.size <= 256:  # (the library's banks end at BLAH2HIP_MAX_RATES; the restatement's need not)
        raise ValueError("a bank holds 1 .. 256 rates")
    h = np.zeros(nD) if half_walk is None else np.asarray(half_walk, dtype=np.float64)
    if h.shape != (nD,):
        raise ValueError("half_walk must hold one entry per Doppler row")
    c = rate_chirps(q, nD)
    every = np.zeros((q.size,) + R.shape, dtype=np.complex128)
    for j, g, w in _walk_rows(R, h):  # gathered once for the whole bank
        for k in range(q.size):
            every[k, ..., j, :] = np.sum(g * (c[k] * w)[:, None], axis=-2)
    index = np.argmax(np.abs(every) ** 2, axis=0).astype(np.uint8)  # the first of equals
    maps = np.take_along_axis(every, index[None].astype(np.int64), axis=0)[0]
    return maps, index, every


class Map:
    """src/data/Map.h: rows = Doppler, cols = delay.  ``data`` is complex64."""

    def __init__(self, owner, data, delay, doppler, noise_power, max_power, cpi_index=0):
        self._owner = owner
        self._cpi_index = cpi_index
        self.data = data
        self.delay = delay
        self.doppler = doppler
        self.noisePower = noise_power
        self.maxPower = max_power
        # which device copy this map mirrors: the engine's process-call counter and a fingerprint of the cells
        # (like Map::fingerprint of the C++ class): the detectors run on the engine's copy only while both still match
        self._gen = getattr(owner, "_gen", None)
        self._fp = self._fingerprint()

    def _fingerprint(self):
        # position-dependent (CRC-32 of the bytes + Adler-32, with the shape): a swap of two cells, a roll or equal edits
        # at two places change it, like the C++ Map::fingerprint
        import zlib
        raw = np.ascontiguousarray(self.data).view(np.uint8).ravel()
        return (zlib.crc32(raw), zlib.adler32(raw), self.data.shape)

    def device_copy_is_current(self) -> bool:
        """True while the engine's device copy is still this map: no later process call on the engine and no change of
        ``data`` by the caller."""
        return self._owner is not None and self._gen == getattr(self._owner, "_gen", None) and self._fp == self._fingerprint()

    def get_nRows(self):
        return self.data.shape[0]

    def get_nCols(self):
        return self.data.shape[1]

    def set_metrics(self):
        """Map::set_metrics (Map.cpp:187-206).  The reduction is fused into the
        Doppler kernel, so the values are already there; kept so that callers
        can follow blah2.cpp:278-279 verbatim."""
        return None


class Detection:
    """src/data/Detection.h:13-70."""

    def __init__(self, delay, doppler, snr):
        self.delay = np.asarray(delay, dtype=np.float64)
        self.doppler = np.asarray(doppler, dtype=np.float64)
        self.snr = np.asarray(snr, dtype=np.float64)

    def get_delay(self):
        return self.delay.copy()

    def get_doppler(self):
        return self.doppler.copy()

    def get_snr(self):
        return self.snr.copy()

    def get_nDetections(self):
        return int(self.delay.size)


class _FirTaps:
    """Given taps for ``Ambiguity.set_fir``: a complex64 device tensor [CPIs][nBins] (anything with torch's ``data_ptr``,
    ``shape``, ``dtype``, ``is_contiguous``) in the place of a WienerHopf handle.  Holds the tensor: the ambiguity handle
    reads its memory on every call."""

    _h = True  # never closed

    def __init__(self, taps, delay_min):
        if len(taps.shape) != 2 or taps.shape[0] < 1 or taps.shape[1] < 1:
            raise ValueError("set_fir: taps of shape [CPIs][nBins]")
        if "complex64" not in str(taps.dtype) or not taps.is_contiguous() or not getattr(taps, "is_cuda", False):
            raise ValueError("set_fir: a contiguous complex64 tensor on the device")
        self.taps = taps
        self.max_batch, self.n_bins = int(taps.shape[0]), int(taps.shape[1])
        self.delay_min = int(delay_min)

    def taps_dev(self):
        return self.taps.data_ptr(), self.n_bins, self.delay_min


class Ambiguity:
    """src/process/ambiguity/Ambiguity.h:34-58."""

    def __init__(self, delayMin, delayMax, dopplerMin, dopplerMax, fs, n, roundHamming=False,
                 device=0, max_batch=1, n_doppler_bins=0):
        """``n_doppler_bins`` (extension): an explicit number of Doppler bins, e.g. exactly 512;
        0 = the reference's rule (always odd)."""
        L = _lib.load()
        h = C.c_void_p()
        check(L.blah2hip_amb_create_ex(delayMin, delayMax, dopplerMin, dopplerMax, fs, n,
                                       1 if roundHamming else 0, n_doppler_bins, device, max_batch, C.byref(h)))
        self._h = h
        self._L = L
        self.device = device
        self.dims = AmbDims()
        check(L.blah2hip_amb_get_dims(h, C.byref(self.dims)))
        self.delay = np.zeros(self.dims.n_delay_bins, dtype=np.int32)
        self.doppler = np.zeros(self.dims.n_doppler_bins, dtype=np.float64)
        check(L.blah2hip_amb_get_axes(h, _ptr(self.delay), _ptr(self.doppler)))
        self._n_samples = n
        self._gen = 0  # process calls so far: a Map remembers which one produced it

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.blah2hip_amb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- getters (Ambiguity.cpp:174-199) --------------------------------------
    def get_doppler_middle(self):
        return self.dims.doppler_middle

    def get_n_delay_bins(self):
        return self.dims.n_delay_bins

    def get_n_doppler_bins(self):
        return self.dims.n_doppler_bins

    def get_n_corr(self):
        return self.dims.n_corr

    def get_cpi(self):
        return self.dims.cpi

    def get_nfft(self):
        return self.dims.nfft

    def get_n_samples(self):
        return self._n_samples

    # -- process --------------------------------------------------------------
    def _result(self, out, met, cpi_index=0):
        return Map(self, out, self.delay.copy(), self.doppler.copy(), float(met[0]), float(met[1]), cpi_index)

    def process(self, x, y):
        """Ambiguity::process (+ Map::set_metrics) on host arrays of complex
        samples (x = reference, y = surveillance).  Like the reference it
        consumes n_corr*n_doppler_bins samples and raises on underflow
        (IqData::pop_front, IqData.cpp:57-59)."""
        x = np.ascontiguousarray(x)
        y = np.ascontiguousarray(y)
        nD, nC = self.dims.n_doppler_bins, self.dims.n_delay_bins
        out = np.empty((nD, nC), dtype=np.complex64)
        met = np.zeros(2, dtype=np.float64)
        if x.dtype == np.complex64 and y.dtype == np.complex64:
            fn = self._L.blah2hip_amb_process_c32
        else:
            x = x.astype(np.complex128, copy=False)
            y = y.astype(np.complex128, copy=False)
            fn = self._L.blah2hip_amb_process_c64
        n = min(x.shape[0], y.shape[0])
        rc = fn(self._h, _ptr(x), _ptr(y), n, _ptr(out), _ptr(met))
        if rc == _lib.ERR_UNDERFLOW:
            raise RuntimeError("Attempting to pop from an empty deque")
        check(rc)
        self._n_samples = self.dims.n_used  # Ambiguity.cpp:105
        self._gen += 1
        return self._result(out, met)

    def process_i16(self, iq):
        """Same, on the .rspduo wire layout: int16 array [n, 4] = I1 Q1 I2 Q2."""
        iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1, 4)
        nD, nC = self.dims.n_doppler_bins, self.dims.n_delay_bins
        out = np.empty((nD, nC), dtype=np.complex64)
        met = np.zeros(2, dtype=np.float64)
        rc = self._L.blah2hip_amb_process_i16(self._h, _ptr(iq), iq.shape[0], _ptr(out), _ptr(met))
        if rc == _lib.ERR_UNDERFLOW:
            raise RuntimeError("Attempting to pop from an empty deque")
        check(rc)
        self._n_samples = self.dims.n_used
        self._gen += 1
        return self._result(out, met)

    def process_i8(self, x, y):
        """Same, on the 8-bit receivers' samples: two int8 arrays [n, 2] = I, Q (FMT_I8), uploaded as they are."""
        x = np.ascontiguousarray(x, dtype=np.int8).reshape(-1, 2)
        y = np.ascontiguousarray(y, dtype=np.int8).reshape(-1, 2)
        if x.shape != y.shape:
            raise ValueError("x and y must hold the same number of samples")
        nD, nC = self.dims.n_doppler_bins, self.dims.n_delay_bins
        out = np.empty((nD, nC), dtype=np.complex64)
        met = np.zeros(2, dtype=np.float64)
        rc = self._L.blah2hip_amb_process_i8(self._h, _ptr(x), _ptr(y), x.shape[0], _ptr(out), _ptr(met))
        if rc == _lib.ERR_UNDERFLOW:
            raise RuntimeError("Attempting to pop from an empty deque")
        check(rc)
        self._n_samples = self.dims.n_used
        self._gen += 1
        return self._result(out, met)

    def process_dev(self, fmt, d_x, d_y, n_cpi, cpi_stride, d_map=None, d_metrics=None, stream=0):
        """Enqueue the device-resident chain on ``stream`` (raw pointers/ints).  ``fmt``: FMT_C32, FMT_F16 or FMT_I8 (two
        planes), FMT_I16 (d_x = the .rspduo words, d_y unused), FMT_I16X_C32Y or FMT_I8X_C32Y (d_x as for FMT_I16 / FMT_I8,
        d_y a complex64 plane: behind the two-stage clutter filter)."""
        fir = getattr(self, "_fir", None)
        if fir is not None:
            if fir._h is None:
                raise Blah2HipError(_lib.ERR_INVALID, "set_fir: the WienerHopf handle has been closed")
            if n_cpi > fir.max_batch:
                raise Blah2HipError(_lib.ERR_INVALID, f"set_fir: {n_cpi} CPIs, the filter handle holds taps for {fir.max_batch}")
        check(self._L.blah2hip_amb_process_dev(self._h, fmt, d_x, d_y, n_cpi, cpi_stride, d_map,
                                               d_metrics, stream))
        self._gen += 1

    def process_multi_dev(self, fmt, d_x, d_ys, n_cpi, cpi_stride, d_map=None, d_metrics=None, stream=0):
        """One reference plane against ``len(d_ys)`` surveillance planes (blah2hip_amb_process_multi_dev; raw pointers/ints).
        ``fmt``: FMT_C32, FMT_F16, FMT_I8, FMT_I16X_C32Y or FMT_I8X_C32Y.  Output channel-major: channel k of CPI c is
        virtual CPI ``k * n_cpi + c`` of the map / metrics buffers, of ``read_last`` and of the detectors' ``process_dev``
        (called with ``n_cpi * len(d_ys)``)."""
        planes = (C.c_void_p * max(1, len(d_ys)))(*[int(p) if p else None for p in d_ys])
        check(self._L.blah2hip_amb_process_multi_dev(self._h, fmt, d_x, planes, len(d_ys), n_cpi, cpi_stride, d_map,
                                                     d_metrics, stream))
        self._gen += 1

    def process_multi(self, x, ys):
        """Host arrays, one CPI: complex64 reference ``x`` against the complex64 surveillance channels ``ys``
        (blah2hip_amb_process_multi_c32); one :class:`Map` per channel."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        ys = [np.ascontiguousarray(y, dtype=np.complex64) for y in ys]
        nD, nC = self.dims.n_doppler_bins, self.dims.n_delay_bins
        out = np.empty((len(ys), nD, nC), dtype=np.complex64)
        met = np.zeros((len(ys), 2), dtype=np.float64)
        planes = (C.c_void_p * max(1, len(ys)))(*[y.ctypes.data for y in ys])
        n = min([x.shape[0]] + [y.shape[0] for y in ys])
        rc = self._L.blah2hip_amb_process_multi_c32(self._h, _ptr(x), planes, len(ys), n, _ptr(out), _ptr(met))
        if rc == _lib.ERR_UNDERFLOW:
            raise RuntimeError("Attempting to pop from an empty deque")
        check(rc)
        self._n_samples = self.dims.n_used
        self._gen += 1
        return [self._result(out[k], met[k], k) for k in range(len(ys))]

    def beamform_dev(self, d_map, n_surv, n_cpi, w, d_beam_map, d_beam_metrics, stream=0):
        """Beams over the channel maps of ``process_multi_dev`` (blah2hip_amb_beamform_dev; raw pointers/ints): ``w`` is a
        complex array ``[n_beams, n_surv]`` (host), ``d_map`` the ``[n_surv][n_cpi]`` maps (None: the handle's own).  Beam b of
        CPI c is virtual CPI ``b * n_cpi + c`` of ``d_beam_map`` / ``d_beam_metrics`` for the detectors' ``process_dev``
        (called with ``n_beams * n_cpi``)."""
        w = np.ascontiguousarray(w, dtype=np.complex64)
        if w.ndim != 2 or w.shape[1] != n_surv:
            raise ValueError("w must be [n_beams, n_surv]")
        check(self._L.blah2hip_amb_beamform_dev(self._h, d_map, n_surv, n_cpi, _ptr(w), w.shape[0], d_beam_map,
                                                d_beam_metrics, stream))

    def beamform_wdev(self, d_map, n_surv, n_cpi, d_w, n_beams, d_beam_map, d_beam_metrics, stream=0):
        """``beamform_dev`` with a set of weights per CPI on the device (blah2hip_amb_beamform_wdev; raw pointers/ints):
        ``d_w`` is complex64 ``[n_cpi][n_beams][n_surv]``, as ``mvdr_weights_dev`` writes it."""
        check(self._L.blah2hip_amb_beamform_wdev(self._h, d_map, n_surv, n_cpi, d_w, n_beams, d_beam_map, d_beam_metrics, stream))

    def covariance_dev(self, d_map, n_surv, n_cpi, d_cov, region=None, stream=0):
        """The array covariance of the channel maps per CPI (blah2hip_amb_covariance_dev; raw pointers/ints): ``d_cov`` is
        complex128 ``[n_cpi][n_surv][n_surv]``, ``R[c][i][j] = sum M_i conj(M_j)`` over the cells of ``region`` =
        ``(row0, row1, col0, col1)`` (None: the whole map)."""
        row0, row1, col0, col1 = region if region is not None else (0, self.dims.n_doppler_bins, 0, self.dims.n_delay_bins)
        check(self._L.blah2hip_amb_covariance_dev(self._h, d_map, n_surv, n_cpi, row0, row1, col0, col1, d_cov, stream))

    def mvdr_weights_dev(self, d_cov, n_surv, n_cpi, steer, loading, d_w, d_ok=None, stream=0):
        """Minimum-variance weights per CPI and beam from ``d_cov`` (blah2hip_amb_mvdr_weights_dev; raw pointers/ints):
        ``steer`` is a complex array ``[n_beams, n_surv]`` (host, e.g. :func:`ula_steering`), ``d_w`` complex64
        ``[n_cpi][n_beams][n_surv]``, ``d_ok`` int32 ``[n_cpi]`` or None.  :func:`mvdr_weights` is the same in NumPy."""
        steer = np.ascontiguousarray(steer, dtype=np.complex64)
        if steer.ndim != 2 or steer.shape[1] != n_surv:
            raise ValueError("steer must be [n_beams, n_surv]")
        check(self._L.blah2hip_amb_mvdr_weights_dev(self._h, d_cov, n_surv, n_cpi, _ptr(steer), steer.shape[0], float(loading),
                                                    d_w, d_ok, stream))

    def adaptive_beamform_dev(self, d_map, n_surv, n_cpi, steer, loading, d_cov, d_w, d_ok, d_beam_map, d_beam_metrics,
                              region=None, stream=0):
        """Adaptive beams, enqueued in order on ``stream``: ``covariance_dev`` over ``region``, ``mvdr_weights_dev`` towards
        ``steer`` (``[n_beams, n_surv]``, host) and ``beamform_wdev`` with the weights it left in ``d_w``.  Beam b of CPI c is
        virtual CPI ``b * n_cpi + c`` of ``d_beam_map`` / ``d_beam_metrics``, as for ``beamform_dev``."""
        steer = np.ascontiguousarray(steer, dtype=np.complex64)
        self.covariance_dev(d_map, n_surv, n_cpi, d_cov, region, stream)
        self.mvdr_weights_dev(d_cov, n_surv, n_cpi, steer, loading, d_w, d_ok, stream)
        self.beamform_wdev(d_map, n_surv, n_cpi, d_w, steer.shape[0], d_beam_map, d_beam_metrics, stream)

    @staticmethod
    def _planes(ptrs):
        return (C.c_void_p * max(1, len(ptrs)))(*[int(p) if p else None for p in ptrs])

    def sample_covariance_dev(self, fmt, d_ys, n_cpi, cpi_stride, d_cov, window=None, stream=0):
        """The array covariance of the channels' SAMPLES per CPI (blah2hip_amb_sample_covariance_dev; raw pointers/ints):
        ``d_ys`` the ``n_surv`` planes (FMT_C32 or FMT_I8), ``d_cov`` complex128 ``[n_cpi][n_surv][n_surv]`` as
        ``covariance_dev`` writes it, over the samples ``window`` = ``(s0, s1)`` of every CPI (None: all of it).
        :func:`sample_covariance` is the same in NumPy."""
        s0, s1 = window if window is not None else (0, self.dims.n_samples)
        check(self._L.blah2hip_amb_sample_covariance_dev(self._h, fmt, self._planes(d_ys), len(d_ys), n_cpi, cpi_stride, s0, s1,
                                                         d_cov, stream))

    def beam_samples_dev(self, fmt, d_ys, n_cpi, cpi_stride, w, d_beams, beam_stride, stream=0):
        """Beam planes from the channels' samples (blah2hip_amb_beam_samples_dev; raw pointers/ints): ``w`` is a complex array
        ``[n_beams, n_surv]`` (host), ``d_beams`` the ``n_beams`` complex64 output planes, CPI c at ``c * beam_stride``
        samples -- each one a ``d_y`` for ``process_dev`` (FMT_C32, FMT_I8X_C32Y, FMT_I16X_C32Y) and for the clutter filter.
        :func:`beam_samples` is the same in NumPy."""
        w = np.ascontiguousarray(w, dtype=np.complex64)
        if w.ndim != 2 or w.shape[1] != len(d_ys) or w.shape[0] != len(d_beams):
            raise ValueError("w must be [n_beams, n_surv]")
        check(self._L.blah2hip_amb_beam_samples_dev(self._h, fmt, self._planes(d_ys), len(d_ys), n_cpi, cpi_stride, _ptr(w),
                                                    len(d_beams), self._planes(d_beams), beam_stride, stream))

    def beam_samples_wdev(self, fmt, d_ys, n_cpi, cpi_stride, d_w, d_beams, beam_stride, stream=0):
        """``beam_samples_dev`` with a set of weights per CPI on the device (blah2hip_amb_beam_samples_wdev; raw
        pointers/ints): ``d_w`` is complex64 ``[n_cpi][n_beams][n_surv]``, as ``mvdr_weights_dev`` writes it."""
        check(self._L.blah2hip_amb_beam_samples_wdev(self._h, fmt, self._planes(d_ys), len(d_ys), n_cpi, cpi_stride, d_w,
                                                     len(d_beams), self._planes(d_beams), beam_stride, stream))

    def adaptive_beam_samples_dev(self, fmt, d_ys, n_cpi, cpi_stride, steer, loading, d_cov, d_w, d_ok, d_beams, beam_stride,
                                  window=None, stream=0):
        """Adaptive beam planes, enqueued in order on ``stream``: ``sample_covariance_dev`` over ``window``,
        ``mvdr_weights_dev`` towards ``steer`` (``[n_beams, n_surv]``, host) and ``beam_samples_wdev`` with the weights it left
        in ``d_w`` -- ``adaptive_beamform_dev`` in front of the range and Doppler stages instead of behind them."""
        steer = np.ascontiguousarray(steer, dtype=np.complex64)
        if steer.ndim != 2 or steer.shape[0] != len(d_beams):
            raise ValueError("steer must be [n_beams, n_surv] with one row per beam plane")
        self.sample_covariance_dev(fmt, d_ys, n_cpi, cpi_stride, d_cov, window, stream)
        self.mvdr_weights_dev(d_cov, len(d_ys), n_cpi, steer, loading, d_w, d_ok, stream)
        self.beam_samples_wdev(fmt, d_ys, n_cpi, cpi_stride, d_w, d_beams, beam_stride, stream)

    def snapshot_dev(self, d_map, n_surv, n_cpi, d_dets, cap, d_count, n_lists, d_snap, stream=0):
        """The ``n_surv`` channel cells under every record of ``n_lists`` detection lists (blah2hip_amb_snapshot_dev; raw
        pointers/ints): ``d_snap`` is complex64 ``[n_lists][cap][n_surv]``, list l reads the channel maps of CPI
        ``l % n_cpi``."""
        check(self._L.blah2hip_amb_snapshot_dev(self._h, d_map, n_surv, n_cpi, d_dets, cap, d_count, n_lists, d_snap, stream))

    def bearing_dev(self, d_map, n_surv, n_cpi, d_dets, cap, d_count, n_lists, d_steer, n_grid, d_out, d_cov=None, loading=0.0,
                    wrap=False, stream=0):
        """A bearing per record of ``n_lists`` detection lists (blah2hip_amb_bearing_dev; raw pointers/ints): the snapshot
        under each record scanned over the DEVICE table ``d_steer`` (complex64 ``[n_grid][n_surv]``), whitened by the CPI's
        covariance ``d_cov`` (complex128 ``[n_cpi][n_surv][n_surv]``, as ``covariance_dev`` writes it) with diagonal
        ``loading`` -- or the Bartlett scan where ``d_cov`` is None.  ``d_out`` is ``[n_lists][cap]`` of
        :data:`BEARING_DTYPE`; list l reads CPI ``l % n_cpi``.  :func:`bearing` is the same in NumPy."""
        check(self._L.blah2hip_amb_bearing_dev(self._h, d_map, n_surv, n_cpi, d_dets, cap, d_count, n_lists, d_cov, float(loading),
                                               d_steer, n_grid, _lib.BEARING_WRAP if wrap else 0, d_out, stream))

    def beamform(self, maps, w):
        """Host arrays, one CPI: the channel maps ``maps`` (:class:`Map` or complex64 ``[n_doppler, n_delay]`` arrays, one per
        channel) combined with ``w`` (complex ``[n_beams, n_surv]``); uploads, runs ``beamform_dev`` and returns one
        :class:`Map` per beam with its metrics."""
        data = np.stack([np.ascontiguousarray(getattr(m, "data", m), dtype=np.complex64) for m in maps])
        w = np.ascontiguousarray(w, dtype=np.complex64)
        nD, nC = self.dims.n_doppler_bins, self.dims.n_delay_bins
        if data.shape[1:] != (nD, nC):
            raise ValueError(f"maps must be [{nD}, {nC}]")
        out = np.empty((w.shape[0], nD, nC), dtype=np.complex64)
        met = np.zeros((w.shape[0], 2), dtype=np.float64)
        L, ctx = self._L, C.c_void_p()
        check(L.blah2hip_ctx_create(self.device, C.byref(ctx)))
        bufs = []
        try:
            for nbytes in (data.nbytes, out.nbytes, met.nbytes):
                p = C.c_void_p()
                check(L.blah2hip_ctx_malloc(ctx, nbytes, C.byref(p)))
                bufs.append(p)
            d_in, d_out, d_met = bufs
            check(L.blah2hip_ctx_h2d(ctx, d_in, _ptr(data), data.nbytes))
            self.beamform_dev(d_in, data.shape[0], 1, w, d_out, d_met, L.blah2hip_ctx_stream(ctx))
            check(L.blah2hip_ctx_d2h(ctx, _ptr(out), d_out, out.nbytes))
            check(L.blah2hip_ctx_d2h(ctx, _ptr(met), d_met, met.nbytes))
            check(L.blah2hip_ctx_sync(ctx))
        finally:
            for p in bufs:
                L.blah2hip_ctx_free(ctx, p)
            L.blah2hip_ctx_destroy(ctx)
        # (a beam map is not the engine's device copy: no owner, so a detector uploads it)
        return [Map(None, out[b], self.delay.copy(), self.doppler.copy(), float(met[b, 0]), float(met[b, 1]), b)
                for b in range(w.shape[0])]

    def set_multi_surv_range(self, mode):
        """BLAH2HIP_OPT_MULTI_SURV_RANGE: "auto", "shared" (the shared-reference range kernel) or "per_channel"."""
        mode = {"auto": _lib.MULTI_AUTO, "shared": _lib.MULTI_SHARED, "per_channel": _lib.MULTI_PER_CHANNEL}.get(mode, mode)
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_MULTI_SURV_RANGE, int(mode)))

    def set_cfar_looks(self, looks):
        """BLAH2HIP_OPT_CFAR_LOOKS: the looks per cell the detectors' threshold factors are made for, 1 (default) for the
        engine's own maps, ``n_surv * window`` for the maps of a :class:`MapIntegrator` (its ``looks``).  The detector
        classes set it from their own ``looks`` at every call."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_CFAR_LOOKS, int(looks)))

    def read_last(self, cpi=0):
        nD, nC = self.dims.n_doppler_bins, self.dims.n_delay_bins
        out = np.empty((nD, nC), dtype=np.complex64)
        met = np.zeros(2, dtype=np.float64)
        check(self._L.blah2hip_amb_read_last(self._h, cpi, _ptr(out), _ptr(met)))
        return self._result(out, met, cpi)

    def db_dev(self, d_map, d_metrics, n_cpi, d_db, stream=0):
        """Enqueue the fp32 dB map Map::to_json prints (10*log10|M| - noisePower) for n_cpi maps."""
        check(self._L.blah2hip_amb_db_dev(self._h, d_map, d_metrics, n_cpi, d_db, stream))

    # -- execution plan (engine-specific, not part of the reference surface) ----
    def set_doppler_kernel(self, which):
        """Force one of the Doppler kernels (``_lib.DOP_*`` or its name); 'auto' picks by launch size."""
        if isinstance(which, str):
            which = {v: k for k, v in _lib.DOPPLER_KERNEL_NAMES.items()}[which]
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_DOPPLER_KERNEL, int(which)))

    def set_range_grid(self, n):
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_RANGE_GRID, int(n)))

    def set_range_walk(self, which):
        """Pulse walk of the one-wave 1024-point range kernel: ``_lib.WALK_AUTO`` (the engine's choice), ``_STATIC``
        or ``_TICKET`` (or 'auto' / 'static' / 'ticket').  The results are the same bits."""
        if isinstance(which, str):
            which = {"auto": _lib.WALK_AUTO, "static": _lib.WALK_STATIC, "ticket": _lib.WALK_TICKET}[which]
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_RANGE_WALK, int(which)))

    def set_doppler_grid(self, n):
        """Workgroup cap of the persistent Doppler tile kernels (0 = their residency)."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_DOPPLER_GRID, int(n)))

    def set_cfar2d_kernel(self, which):
        """'auto' / 'tile' (one pass over the map) / 'sat' (summed-area table) for :class:`CfarDetector2D`."""
        if isinstance(which, str):
            which = {"auto": _lib.CFAR2D_AUTO, "tile": _lib.CFAR2D_TILE, "sat": _lib.CFAR2D_SAT, "stream": _lib.CFAR2D_STREAM}[which]
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_CFAR2D_KERNEL, int(which)))

    def set_cfar2d_seg_rows(self, n):
        """Doppler rows per segment of the 2-D stream kernel (0 = its cost model); ``info(INFO_CFAR2D_SEG_ROWS)`` reports
        what the last launch used."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_CFAR2D_SEG_ROWS, int(n)))

    def taper_dev(self, d_map, n_maps, taps, d_out_map, d_out_metrics, stream=0):
        """The Doppler stencil ``taps`` (``t_0 .. t_P``, host, rounded to fp32: :func:`doppler_taper`) over ``n_maps`` maps on
        the device (blah2hip_amb_taper_dev; raw pointers/ints): ``d_map`` None is the handle's own map; the outputs are
        ``[n_maps][nD][nDelay]`` complex64 and ``[n_maps][2]`` float64 and must not overlap the input.  Enqueues only."""
        t = np.ascontiguousarray(taps, dtype=np.float32)
        if t.ndim != 1 or t.size < 1:
            raise ValueError("taps must be t_0 .. t_P")
        check(self._L.blah2hip_amb_taper_dev(self._h, d_map, n_maps, _ptr(t), t.size - 1, d_out_map, d_out_metrics, stream))

    def set_migration(self, half_walk):
        """The table of fp64 half walks (``[n_doppler_bins]``: :func:`migration_table`, or any finite table) that
        :meth:`migrate_dev` sums along (blah2hip_amb_set_migration); None clears it."""
        if half_walk is None:
            check(self._L.blah2hip_amb_set_migration(self._h, None))
            return
        t = np.ascontiguousarray(half_walk, dtype=np.float64)
        if t.shape != (self.dims.n_doppler_bins,):
            raise ValueError("half_walk must hold one entry per Doppler row")
        check(self._L.blah2hip_amb_set_migration(self._h, _ptr(t)))

    def migration_table(self, fc):
        """blah2hip_migration_table: the library's own physical table for the carrier ``fc`` (Hz)."""
        t = np.zeros(self.dims.n_doppler_bins, dtype=np.float64)
        check(self._L.blah2hip_migration_table(self._h, float(fc), _ptr(t)))
        return t

    def migrate_dev(self, d_map, n_maps, d_out_map, d_out_metrics, stream=0):
        """Range-migration compensation of the first ``n_maps`` maps of the last ``process_dev`` / ``process_multi_dev`` call
        (blah2hip_amb_migrate_dev; raw pointers/ints): ``d_map`` is that call's map buffer (None: the handle's own),
        ``d_out_map`` the same pointer or a disjoint ``[n_maps][nD][nDelay]`` complex64 buffer, ``d_out_metrics``
        ``[n_maps][2]`` float64.  Enqueues only."""
        check(self._L.blah2hip_amb_migrate_dev(self._h, d_map, n_maps, d_out_map, d_out_metrics, stream))

    def carrier_table(self, ratio, interp="nearest"):
        """blah2hip_carrier_table: the library's own table that aligns carriers of ``ratio[c] = fc_c / fc_ref`` with this
        handle's Doppler axis, as :func:`carrier_table` returns it."""
        r = np.ascontiguousarray(np.atleast_1d(ratio), dtype=np.float64)
        if r.ndim != 1:
            raise ValueError("ratio is a list of carrier ratios")
        shape = (r.size, self.dims.n_doppler_bins)
        row, a_lo, a_hi = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
        covered = np.zeros(shape[1], dtype=np.uint32)
        check(self._L.blah2hip_carrier_table(self._h, _ptr(r), r.size, _carrier_interp(interp), _ptr(row), _ptr(a_lo), _ptr(a_hi),
                                             _ptr(covered)))
        return {"row": row, "a_lo": a_lo, "a_hi": a_hi, "covered": covered}

    def set_carriers(self, ratio, interp="nearest"):
        """The carrier ratios (at most 8, each in [0.5, 2]) whose table :meth:`fuse_carriers_dev` sums along
        (blah2hip_amb_set_carriers; waits for the device); None or an empty list clears it."""
        if ratio is None or np.size(ratio) == 0:
            check(self._L.blah2hip_amb_set_carriers(self._h, None, 0, 0))
            return
        r = np.ascontiguousarray(np.atleast_1d(ratio), dtype=np.float64)
        if r.ndim != 1:
            raise ValueError("ratio is a list of carrier ratios")
        check(self._L.blah2hip_amb_set_carriers(self._h, _ptr(r), r.size, _carrier_interp(interp)))
        self._n_carriers = r.size

    def fuse_carriers_dev(self, d_map, n_cpi, d_out_map, d_out_metrics, w=None, stream=0):
        """The carriers' maps summed on this handle's Doppler axis (blah2hip_amb_fuse_carriers_dev; raw pointers/ints):
        ``d_map`` is ``[C][n_cpi][nD][nDelay]`` complex64 (None: the handle's own map behind a process call of ``C n_cpi``
        CPIs), ``w`` the ``C`` carrier weights on the host (None: all 1), the outputs ``[n_cpi][nD][nDelay]`` complex64 and
        ``[n_cpi][2]`` float64, which must not overlap the input.  Enqueues only."""
        wp = None
        if w is not None:
            wk = np.ascontiguousarray(w, dtype=np.float32)
            if wk.shape != (getattr(self, "_n_carriers", -1),):
                raise ValueError("w must hold one weight per carrier of the table that is set")
            wp = _ptr(wk)
        check(self._L.blah2hip_amb_fuse_carriers_dev(self._h, d_map, n_cpi, wp, d_out_map, d_out_metrics, stream))

    def doppler_rate(self, fc, accel):
        """blah2hip_doppler_rate: the Doppler rate in bins drifted over this handle's CPI for the carrier ``fc`` (Hz) and the
        second derivative ``accel`` of the bistatic range (m/s^2)."""
        q = C.c_double()
        check(self._L.blah2hip_doppler_rate(self._h, float(fc), float(accel), C.byref(q)))
        return q.value

    def set_rates(self, q):
        """The bank of fp64 Doppler rates (bins drifted over the CPI: :func:`rate_bank`, :func:`doppler_rate`, at most 16) that
        :meth:`rate_bank_dev` tries per cell (blah2hip_amb_set_rates); None or an empty list clears it."""
        if q is None or np.size(q) == 0:
            check(self._L.blah2hip_amb_set_rates(self._h, None, 0))
            return
        t = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
        if t.ndim != 1:
            raise ValueError("the bank is a list of rates")
        check(self._L.blah2hip_amb_set_rates(self._h, _ptr(t), t.size))

    def rate_bank_dev(self, d_map, n_maps, d_out_map, d_out_index, d_out_metrics, stream=0):
        """The Doppler-rate bank over the first ``n_maps`` maps of the last ``process_dev`` / ``process_multi_dev`` call, along
        the walk of the migration table if one is set (blah2hip_amb_rate_bank_dev; raw pointers/ints): ``d_map`` is that
        call's map buffer (None: the handle's own), ``d_out_map`` the same pointer or a disjoint ``[n_maps][nD][nDelay]``
        complex64 buffer, ``d_out_index`` ``[n_maps][nD][nDelay]`` uint8 or None, ``d_out_metrics`` ``[n_maps][2]`` float64.
        Enqueues only."""
        check(self._L.blah2hip_amb_rate_bank_dev(self._h, d_map, n_maps, d_out_map, d_out_index, d_out_metrics, stream))

    def set_taper_seg_rows(self, n):
        """Doppler rows per segment of the taper kernel (0 = the launch's own choice); ``info(INFO_TAPER_GRID)`` reports the
        workgroups per map of the last launch."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_TAPER_SEG_ROWS, int(n)))

    def set_cfar2d_grid(self, n):
        """Workgroup cap of the persistent 2-D tile kernel (0 = one per CU); ``info(INFO_CFAR2D_GRID)`` reports the grid of
        the last launch."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_CFAR2D_GRID, int(n)))

    def set_fir(self, wiener_hopf, delay_min=None):
        """Run the clutter filter's FIR fused into the range kernel with the taps of ``wiener_hopf`` (a WienerHopf whose
        ``estimate_dev_fmt`` precedes each ``process_dev`` on the same stream); None: back to the plain range kernels.
        With ``delay_min`` given, ``wiener_hopf`` is instead a contiguous complex64 device tensor [CPIs][nBins] of taps, tap k
        of a row at lag ``delay_min + k``: given taps, no estimate (a row per CPI of the calls that follow)."""
        if wiener_hopf is None:
            check(self._L.blah2hip_amb_set_fir(self._h, None, 0, 0))
        else:
            if delay_min is None and getattr(wiener_hopf, "blocks", 1) > 1:
                raise ValueError(_FIR_BLOCKS_REASON)
            if delay_min is not None:
                wiener_hopf = _FirTaps(wiener_hopf, delay_min)
            p, nb, dm = wiener_hopf.taps_dev()
            check(self._L.blah2hip_amb_set_fir(self._h, p, nb, dm))
        # the ambiguity handle reads the filter handle's device array on every call: keep it alive, and remember how many
        # CPIs' taps it holds
        self._fir = wiener_hopf

    def fir_fusable(self, wiener_hopf, fmt, delay_min=None):
        """None if ``set_fir(wiener_hopf)`` is covered for samples in format ``fmt`` (FMT_C32 / FMT_I16), else the reason
        (always one for FMT_I8: the fused kernel has no int8 form, an 8-bit chain runs the two-stage filter).  With
        ``delay_min`` given, ``wiener_hopf`` is the number of taps (or a tensor of taps as for ``set_fir``)."""
        if delay_min is None:
            if getattr(wiener_hopf, "blocks", 1) > 1:
                return _FIR_BLOCKS_REASON
            _, nb, dm = wiener_hopf.taps_dev()
        else:
            nb = int(wiener_hopf) if isinstance(wiener_hopf, (int, np.integer)) else _FirTaps(wiener_hopf, delay_min).n_bins
            dm = int(delay_min)
        rc = self._L.blah2hip_amb_fir_fusable(self._h, int(fmt), nb, dm)
        if rc == _lib.OK:
            return None
        if rc == _lib.ERR_UNSUPPORTED:
            return self._L.blah2hip_last_error().decode()
        check(rc)

    def set_hot_columns(self, mode):
        """BLAH2HIP_OPT_HOT_COLUMNS: "off", "auto" (default) or "always" -- the fp64 Doppler transform of the delay columns
        under the map's tallest peaks (include/blah2hip.h)."""
        mode = {"off": 0, "auto": 1, "always": 2}.get(mode, mode)
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_HOT_COLUMNS, int(mode)))

    def hot_columns(self):
        """Columns of the last call's first CPI that were transformed again in fp64 (waits for the device)."""
        return self.info(_lib.INFO_HOT_COLUMNS)

    def hot_columns_missed(self):
        """The most columns of any CPI of the last call that qualified for the fp64 transform and kept their fp32 values (beyond
        the 16 a CPI, or beyond 64 candidates in one quarter of the lags); waits for the device."""
        return self.info(_lib.INFO_HOT_COLUMNS_MISSED)

    def set_leak_compensation(self, mode):
        """BLAH2HIP_OPT_LEAK_COMPENSATION: "off", "auto" (default) or "always" (include/blah2hip.h)."""
        mode = {"off": _lib.LEAK_OFF, "auto": _lib.LEAK_AUTO, "always": _lib.LEAK_ALWAYS}.get(mode, mode)
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_LEAK_COMPENSATION, int(mode)))

    def leak_info(self):
        """(cells of the zero-Doppler row the last call corrected, largest |g| of the kernel pair it ran)."""
        return self.info(_lib.INFO_LEAK_LAGS), self.info(_lib.INFO_LEAK_MAX_E12) * 1e-12

    def set_fft_len(self, F):
        """Force the range transform length (1024 / 2048 / 4096; 0 = planner); re-plans the segmentation."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_FFT_LEN, int(F)))
        check(self._L.blah2hip_amb_get_dims(self._h, C.byref(self.dims)))

    def set_range_kernel(self, which):
        """0 = by transform length, ``_lib.RANGE_WAVE`` = the one-wave kernel (F = 2048 only)."""
        check(self._L.blah2hip_amb_set_option(self._h, _lib.OPT_RANGE_KERNEL, int(which)))

    def info(self, key):
        v = C.c_int64(0)
        check(self._L.blah2hip_amb_get_info(self._h, key, C.byref(v)))
        return v.value

    def last_doppler_kernel(self):
        return _lib.DOPPLER_KERNEL_NAMES[self.info(_lib.INFO_LAST_DOPPLER_KERNEL)]

    # -- per-kernel timing -----------------------------------------------------
    def set_timing(self, enable=True):
        check(self._L.blah2hip_amb_set_timing(self._h, 1 if enable else 0))

    def get_timing(self):
        ms = np.zeros(_lib.K_COUNT, dtype=np.float64)
        cnt = np.zeros(_lib.K_COUNT, dtype=np.uint32)
        check(self._L.blah2hip_amb_get_timing(self._h, _ptr(ms), _ptr(cnt)))
        return {name: (float(ms[k]), int(cnt[k])) for k, name in _lib.KERNEL_NAMES.items()}


class _Cfar:
    """What the four detectors share.  A subclass names its entry points (``_entry`` + ``_process`` / ``_dev``) and gives
    its own arguments in ``_args()``, in the order every entry point of the library takes them."""

    _entry = None

    def _init(self, pfa, minDelay, minDoppler, looks, int8=()):
        for name, v in int8:
            if not -128 <= int(v) <= 127:  # int8_t in the reference
                raise ValueError(f"{name} outside int8 range")
        if not 1 <= int(looks) <= _lib.MAX_CFAR_LOOKS:
            raise ValueError("looks outside [1, MAX_CFAR_LOOKS]")
        self.pfa, self.minDelay, self.minDoppler, self.looks = float(pfa), int(minDelay), float(minDoppler), int(looks)

    def _process_device_copy(self, amb, x):
        """``*_process`` on the map the engine still holds on the device."""
        cap = x.data.size
        d, f, s = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        n = C.c_uint32(0)
        amb.set_cfar_looks(self.looks)
        check(getattr(amb._L, self._entry + "_process")(amb._h, x._cpi_index, *self._args(), _ptr(d), _ptr(f), _ptr(s), cap,
                                                        C.byref(n)))
        k = n.value
        return Detection(d[:k].copy(), f[:k].copy(), s[:k].copy())

    def process_dev(self, amb, n_cpi, d_hits, cap, d_count, d_map=None, d_metrics=None, stream=0):
        """Enqueue the detector for n_cpi device-resident maps (None = the engine's internal buffers of the
        last process_dev): hit records into d_hits [n_cpi][cap], counts into d_count [n_cpi]."""
        amb.set_cfar_looks(self.looks)
        check(getattr(amb._L, self._entry + "_dev")(amb._h, d_map, d_metrics, n_cpi, *self._args(), d_hits, cap, d_count, stream))


class CfarDetector1D(_Cfar):
    """src/process/detection/CfarDetector1D.h:46-55."""

    _entry = "blah2hip_cfar1d"

    def __init__(self, pfa, nGuard, nTrain, minDelay, minDoppler, looks=1):
        """``looks`` (extension): the looks per cell of the maps this detector runs on -- 1 for the engine's maps,
        ``MapIntegrator.looks`` for integrated ones; the detector sets the handle's BLAH2HIP_OPT_CFAR_LOOKS to it at
        every call."""
        self._init(pfa, minDelay, minDoppler, looks, (("nGuard", nGuard), ("nTrain", nTrain), ("minDelay", minDelay)))
        self.nGuard, self.nTrain = int(nGuard), int(nTrain)

    def _args(self):
        return (self.pfa, self.nGuard, self.nTrain, self.minDelay, self.minDoppler)

    def process(self, x: Map) -> Detection:
        """CfarDetector1D::process on ``x.data`` (CfarDetector1D.cpp:23-100).  While ``x`` is still the map the engine holds
        on the device (no later process call, cells untouched) it runs there without an upload; any other Map -- built or
        modified by the caller, or outlived by a newer CPI -- is uploaded and runs through the same kernel
        (blah2hip_cfar1d_map), like the C++ class does."""
        amb = x._owner
        if x.device_copy_is_current():
            return self._process_device_copy(amb, x)
        if self.looks != 1:
            raise ValueError("CfarDetector1D.process: a map held by the host runs through blah2hip_cfar1d_map, which is "
                             "one-look; run process_dev on the integrated maps on the device")
        cap = x.data.size
        d, f, s = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        n = C.c_uint32(0)
        L = _lib.load()
        m = np.ascontiguousarray(x.data, dtype=np.complex64)
        dax = np.ascontiguousarray(x.delay, dtype=np.int32)
        fax = np.ascontiguousarray(x.doppler, dtype=np.float64)
        dev = amb.device if amb is not None else 0
        check(L.blah2hip_cfar1d_map(_ptr(m), m.shape[0], m.shape[1], _ptr(dax), _ptr(fax), float(x.noisePower), self.pfa,
                                    self.nGuard, self.nTrain, self.minDelay, self.minDoppler, dev, _ptr(d), _ptr(f),
                                    _ptr(s), cap, C.byref(n)))
        k = n.value
        return Detection(d[:k].copy(), f[:k].copy(), s[:k].copy())


def hits_to_detection(amb, hits, count, cap):
    """One CPI's device hit records (``blah2hip_hit_t``: int32 row, int32 col, double snr; arbitrary
    order) -> :class:`Detection` in the reference's row-major emission order
    (CfarDetector1D.cpp:36-92: delay = col + delay[0], doppler = doppler[row])."""
    if count > cap:
        raise Blah2HipError(_lib.ERR_CAPACITY, f"{count} detections, capacity {cap}")
    h = np.asarray(hits[:count])
    order = np.lexsort((h["col"], h["row"]))
    h = h[order]
    return Detection(h["col"].astype(np.float64) + float(amb.delay[0]), amb.doppler[h["row"]], h["snr"].astype(np.float64))


HIT_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("snr", np.float64)])


class CfarDetector2D(_Cfar):
    """2-D cell-averaging CFAR (BASELINE.json configs[2]).  Not a reference class:
    the reference only has the 1-D detector; this is its extension as defined in
    SURVEY.md section 8g, and with nGuardDoppler = nTrainDoppler = 0 it returns
    exactly what :class:`CfarDetector1D` returns."""

    _entry = "blah2hip_cfar2d"

    def __init__(self, pfa, nGuardDelay, nTrainDelay, nGuardDoppler, nTrainDoppler, minDelay, minDoppler, looks=1):
        self._init(pfa, minDelay, minDoppler, looks)  # looks: as for CfarDetector1D
        self.p = [int(nGuardDelay), int(nTrainDelay), int(nGuardDoppler), int(nTrainDoppler)]

    def _args(self):
        return (self.pfa, *self.p, self.minDelay, self.minDoppler)

    def process(self, x: Map) -> Detection:
        if not x.device_copy_is_current():
            raise ValueError("CfarDetector2D.process: this Map is no longer the engine's device copy (a later process call, or "
                             "its cells were changed); the 2-D detector has no host-map entry point")
        return self._process_device_copy(x._owner, x)


def _rank_permille(rank):
    """A rank given as a fraction of the training cells (0.75) in the library's unit, 1 .. 1000."""
    pm = int(round(float(rank) * 1000.0))
    if not 1 <= pm <= 1000:
        raise ValueError("rank outside [0.001, 1]")
    return pm


def _detect_host_map(amb, x, enqueue):
    """A detector's ``*_dev`` entry point on a map held by the host: uploads ``x.data`` and ``x.noisePower`` beside a hit
    list of the map's size, runs ``enqueue(d_map, d_metrics, d_hits, cap, d_count, stream)`` and returns the hits in the
    reference's emission order.  ``amb`` gives the geometry and the axes; the map must have its shape."""
    data = np.ascontiguousarray(x.data, dtype=np.complex64)
    if data.shape != (amb.dims.n_doppler_bins, amb.dims.n_delay_bins):
        raise ValueError(f"the map must be [{amb.dims.n_doppler_bins}, {amb.dims.n_delay_bins}]")
    met = np.array([float(x.noisePower), float(x.maxPower)], dtype=np.float64)
    cap = data.size
    hits = np.zeros(cap, dtype=HIT_DTYPE)
    cnt = np.zeros(1, dtype=np.uint32)
    L, ctx = amb._L, C.c_void_p()
    check(L.blah2hip_ctx_create(amb.device, C.byref(ctx)))
    bufs = []
    try:
        for nbytes in (data.nbytes, met.nbytes, hits.nbytes, cnt.nbytes):
            p = C.c_void_p()
            check(L.blah2hip_ctx_malloc(ctx, nbytes, C.byref(p)))
            bufs.append(p)
        d_map, d_met, d_hits, d_cnt = bufs
        check(L.blah2hip_ctx_h2d(ctx, d_map, _ptr(data), data.nbytes))
        check(L.blah2hip_ctx_h2d(ctx, d_met, _ptr(met), met.nbytes))
        enqueue(d_map, d_met, d_hits, cap, d_cnt, L.blah2hip_ctx_stream(ctx))
        check(L.blah2hip_ctx_d2h(ctx, _ptr(cnt), d_cnt, cnt.nbytes))
        check(L.blah2hip_ctx_d2h(ctx, _ptr(hits), d_hits, hits.nbytes))
        check(L.blah2hip_ctx_sync(ctx))
    finally:
        for p in bufs:
            L.blah2hip_ctx_free(ctx, p)
        L.blah2hip_ctx_destroy(ctx)
    return hits_to_detection(amb, hits, int(cnt[0]), cap)


class _OsCfar(_Cfar):
    """The ordered-statistic detectors: a rank, and a ``process`` that also takes maps held by the host."""

    def _process_any(self, x, amb):
        """The device copy while ``x`` still is that map, else an upload of ``x.data``."""
        amb = amb if amb is not None else x._owner
        if x._owner is amb and x.device_copy_is_current():
            return self._process_device_copy(amb, x)
        return _detect_host_map(amb, x, lambda d_map, d_met, d_hits, cap, d_cnt, st:
                                self.process_dev(amb, 1, d_hits, cap, d_cnt, d_map, d_met, st))


class OsCfarDetector1D(_OsCfar):
    """Ordered-statistic CFAR along delay (blah2hip_oscfar1d_*): the geometry of :class:`CfarDetector1D`, the threshold
    ``alpha[n]`` times the k-th smallest training cell, ``k = oscfar_rank(n, 1000 rank)``.  No reference class.
    :func:`oscfar_hits` is the same rule in NumPy."""

    _entry = "blah2hip_oscfar1d"

    def __init__(self, pfa, nGuard, nTrain, minDelay, minDoppler, rank=0.75, looks=1):
        self._init(pfa, minDelay, minDoppler, looks, (("nGuard", nGuard), ("nTrain", nTrain), ("minDelay", minDelay)))
        self.nGuard, self.nTrain = int(nGuard), int(nTrain)
        self.rank_permille = _rank_permille(rank)

    def _args(self):
        return (self.pfa, self.rank_permille, self.nGuard, self.nTrain, self.minDelay, self.minDoppler)

    def process(self, x: Map, amb=None) -> Detection:
        """On the engine's device copy while ``x`` still is that map, else on an upload of ``x.data`` (``amb``: the handle
        that gives the geometry when the map has no owner)."""
        return self._process_any(x, amb)

    def process_dev(self, amb, n_cpi, d_hits, cap, d_count, d_map=None, d_metrics=None, stream=0):
        """Enqueue the detector for n_cpi device-resident maps, like :meth:`CfarDetector1D.process_dev`."""
        super().process_dev(amb, n_cpi, d_hits, cap, d_count, d_map, d_metrics, stream)


class OsCfarDetector2D(_OsCfar):
    """Ordered-statistic CFAR over the window of :class:`CfarDetector2D` (blah2hip_oscfar2d_*); with nGuardDoppler =
    nTrainDoppler = 0 it returns what :class:`OsCfarDetector1D` returns.  Windows beyond a halo of 40 delay columns or 24
    Doppler rows are refused (ERR_UNSUPPORTED)."""

    _entry = "blah2hip_oscfar2d"

    def __init__(self, pfa, nGuardDelay, nTrainDelay, nGuardDoppler, nTrainDoppler, minDelay, minDoppler, rank=0.75, looks=1):
        self._init(pfa, minDelay, minDoppler, looks)
        self.p = [int(nGuardDelay), int(nTrainDelay), int(nGuardDoppler), int(nTrainDoppler)]
        self.rank_permille = _rank_permille(rank)

    def _args(self):
        return (self.pfa, self.rank_permille, *self.p, self.minDelay, self.minDoppler)

    def process(self, x: Map, amb=None) -> Detection:
        return self._process_any(x, amb)


class _GoCfar(_OsCfar):
    """The greatest-of / smallest-of detectors: a kind, one look per cell, and :class:`_OsCfar`'s ``process``."""

    def _init_kind(self, kind, looks):
        if int(looks) != 1:
            raise ValueError("looks: the greatest-of / smallest-of thresholds are made for one look per cell")
        self.kind = gocfar_kind(kind)


class GoCfarDetector1D(_GoCfar):
    """Greatest-of (``kind="go"``) or smallest-of (``"so"``) CFAR along delay (blah2hip_gocfar1d_*): the geometry of
    :class:`CfarDetector1D`, the cell against the mean of each half of its window on its own.  No reference class.
    :func:`gocfar_hits` is the same rule in NumPy."""

    _entry = "blah2hip_gocfar1d"

    def __init__(self, pfa, nGuard, nTrain, minDelay, minDoppler, kind="go", looks=1):
        self._init(pfa, minDelay, minDoppler, looks, (("nGuard", nGuard), ("nTrain", nTrain), ("minDelay", minDelay)))
        self._init_kind(kind, looks)
        self.nGuard, self.nTrain = int(nGuard), int(nTrain)

    def _args(self):
        return (self.pfa, self.kind, self.nGuard, self.nTrain, self.minDelay, self.minDoppler)

    def prepare(self, amb):
        """Build and pin the table on ``amb`` (blah2hip_gocfar1d_prepare): the call to make before capturing a graph."""
        amb.set_cfar_looks(self.looks)
        check(amb._L.blah2hip_gocfar1d_prepare(amb._h, self.pfa, self.kind, self.nGuard, self.nTrain))

    def process(self, x: Map, amb=None) -> Detection:
        """On the engine's device copy while ``x`` still is that map, else on an upload of ``x.data`` (``amb``: the handle
        that gives the geometry when the map has no owner)."""
        return self._process_any(x, amb)


class GoCfarDetector2D(_GoCfar):
    """Greatest-of / smallest-of CFAR with the halves of :class:`GoCfarDetector1D` averaged over ``nRowsDoppler`` rows on
    either side (blah2hip_gocfar2d_*); with ``nRowsDoppler = 0`` it returns what the 1-D detector returns.  Windows beyond
    ``nRowsDoppler <= 24``, ``nGuardDelay + nTrainDelay <= 40`` are refused (ERR_UNSUPPORTED)."""

    _entry = "blah2hip_gocfar2d"

    def __init__(self, pfa, nGuardDelay, nTrainDelay, nRowsDoppler, minDelay, minDoppler, kind="go", looks=1):
        self._init(pfa, minDelay, minDoppler, looks)
        self._init_kind(kind, looks)
        self.p = [int(nGuardDelay), int(nTrainDelay), int(nRowsDoppler)]

    def _args(self):
        return (self.pfa, self.kind, *self.p, self.minDelay, self.minDoppler)

    def prepare(self, amb):
        amb.set_cfar_looks(self.looks)
        check(amb._L.blah2hip_gocfar2d_prepare(amb._h, self.pfa, self.kind, *self.p))

    def process(self, x: Map, amb=None) -> Detection:
        return self._process_any(x, amb)


class MapIntegrator:
    """Non-coherent integration of the maps of ``amb`` over its ``n_surv`` surveillance channels and over a sliding window
    of ``window`` consecutive CPIs, a window every ``hop`` CPIs (None: 1) -- blah2hip_nci_*.  No reference counterpart.
    The output maps are ordinary complex maps (RMS level, zero imaginary part) with ``looks`` = ``n_surv * window`` looks
    per cell: run the detectors on them with ``looks=integrator.looks``.  The CPI counter and the history of the last
    ``window - 1`` CPIs carry over from call to call; ``close()`` it before its ``amb``."""

    def __init__(self, amb, n_surv=1, window=1, hop=None):
        h = C.c_void_p()
        hop = 1 if hop is None else hop
        check(amb._L.blah2hip_nci_create(amb._h, int(n_surv), int(window), int(hop), C.byref(h)))
        self._h, self._L, self.amb = h, amb._L, amb
        self.n_surv, self.window, self.hop = int(n_surv), int(window), int(hop)
        self.looks = self.n_surv * self.window
        self.n_rates = 0  # hypotheses of the tracks that are set (0: none, the plain window sum)

    def set_tracks(self, walk=None, q=None, max_cpi=1):
        """Integrate along tracks from now on (blah2hip_nci_set_tracks): ``walk [n_doppler]`` delay cells an echo of each row
        moves later per CPI (None: zero; :func:`nci_walk_table` is the physical table), ``q`` the bank of Doppler rows it
        rises per CPI (None: ``{0}``), ``max_cpi`` the most CPIs one ``process_tracks_dev`` call brings.  Waits for the
        device, resets the counter.  A cell of the output is the largest of ``n_rates`` sums of ``looks`` looks: make the
        detector with ``looks`` and ``pfa / n_rates``."""
        nD = self.amb.dims.n_doppler_bins
        wp = qp = None
        n_q = 0
        if walk is not None:
            walk = np.ascontiguousarray(walk, dtype=np.float64)
            if walk.shape != (nD,):
                raise ValueError(f"walk must hold {nD} entries, one per Doppler row")
            wp = _ptr(walk)
        if q is not None and np.size(q):
            q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
            if q.ndim != 1:
                raise ValueError("q must be a bank of rates")
            qp, n_q = _ptr(q), q.size
        check(self._L.blah2hip_nci_set_tracks(self._h, wp, qp, n_q, int(max_cpi)))
        self.n_rates = max(n_q, 1)

    def process_tracks_dev(self, d_map, n_cpi, d_out_map, d_out_index, d_out_metrics, out_cap, w=None, stream=0):
        """``process_dev`` along the tracks (blah2hip_nci_process_tracks_dev): the same arguments and return value, with
        ``d_out_index`` the uint8 plane ``[n_out][n_doppler][n_delay]`` of winning hypotheses, or None."""
        wp = None
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (self.n_surv,):
                raise ValueError("w must hold one weight per channel")
            wp = _ptr(w)
        n, f = C.c_uint32(0), C.c_uint64(0)
        check(self._L.blah2hip_nci_process_tracks_dev(self._h, d_map, int(n_cpi), wp, d_out_map, d_out_index, d_out_metrics,
                                                      int(out_cap), C.byref(n), C.byref(f), stream))
        return n.value, f.value

    def close(self):
        if getattr(self, "_h", None):
            # the integrator reads its ambiguity handle when it is destroyed: once that handle is closed (the wrong order)
            # the history planes are left to the process rather than freed through a dangling pointer
            if getattr(self.amb, "_h", None):
                self._L.blah2hip_nci_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Counter 0, history forgotten (host only)."""
        check(self._L.blah2hip_nci_reset(self._h))

    def set_timing(self, enable=True):
        """Bracket every launch of the integrator's kernel with an event pair (blah2hip_nci_set_timing)."""
        check(self._L.blah2hip_nci_set_timing(self._h, 1 if enable else 0))

    def get_timing(self):
        """``{"nci": (ms, launches)}`` since the last call (synchronises); the metrics kernel behind it counts under the
        ambiguity handle's ``"metrics"``.  With tracks set also ``"track_power"`` and ``"track_sum"``, the two kernels of
        ``process_tracks_dev``."""
        ms = np.zeros(_lib.NK_COUNT, dtype=np.float64)
        cnt = np.zeros(_lib.NK_COUNT, dtype=np.uint32)
        check(self._L.blah2hip_nci_get_timing(self._h, _ptr(ms), _ptr(cnt)))
        return {name: (float(ms[k]), int(cnt[k])) for k, name in _lib.NCI_KERNEL_NAMES.items()
                if k == _lib.NK_NCI or self.n_rates}

    def count(self, n_cpi):
        """``(n_out, first_end)`` the next ``process_dev`` of ``n_cpi`` CPIs will report; changes nothing."""
        n, f = C.c_uint32(0), C.c_uint64(0)
        check(self._L.blah2hip_nci_count(self._h, int(n_cpi), C.byref(n), C.byref(f)))
        return n.value, f.value

    def process_dev(self, d_map, n_cpi, d_out_map, d_out_metrics, out_cap, w=None, stream=0):
        """Enqueue the next ``n_cpi`` CPIs (blah2hip_nci_process_dev; raw pointers/ints): ``d_map`` the
        ``[n_surv][n_cpi]`` maps (None: the handle's own), ``w`` the host's channel weights or None, outputs
        ``d_out_map [n_out]`` maps and ``d_out_metrics [n_out][2]`` with room for ``out_cap`` maps.  Returns
        ``(n_out, first_end)``: output i is the window that ends at CPI count ``first_end + i * hop``."""
        wp = None
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (self.n_surv,):
                raise ValueError("w must hold one weight per channel")
            wp = _ptr(w)
        n, f = C.c_uint32(0), C.c_uint64(0)
        check(self._L.blah2hip_nci_process_dev(self._h, d_map, int(n_cpi), wp, d_out_map, d_out_metrics, int(out_cap),
                                               C.byref(n), C.byref(f), stream))
        return n.value, f.value

    def process(self, maps, w=None):
        """Host arrays: complex64 ``maps [n_surv, n_cpi, n_doppler, n_delay]`` (``[n_cpi, ...]`` for one channel), the next
        ``n_cpi`` CPIs; uploads, runs ``process_dev`` and returns one :class:`Map` per window that ended, with its metrics
        and ``cpi_index`` = the CPI count at which it ended."""
        amb = self.amb
        nD, nC = amb.dims.n_doppler_bins, amb.dims.n_delay_bins
        data = np.ascontiguousarray(maps, dtype=np.complex64)
        if data.ndim == 3:
            data = data[None]
        if data.ndim != 4 or data.shape[0] != self.n_surv or data.shape[2:] != (nD, nC):
            raise ValueError(f"maps must be [{self.n_surv}, n_cpi, {nD}, {nC}]")
        n_cpi = data.shape[1]
        n_out, _ = self.count(n_cpi)
        out = np.empty((n_out, nD, nC), dtype=np.complex64)
        met = np.zeros((n_out, 2), dtype=np.float64)
        L, ctx = self._L, C.c_void_p()
        check(L.blah2hip_ctx_create(amb.device, C.byref(ctx)))
        bufs = []
        try:
            for nbytes in (data.nbytes, max(out.nbytes, 16), max(met.nbytes, 16)):
                p = C.c_void_p()
                check(L.blah2hip_ctx_malloc(ctx, nbytes, C.byref(p)))
                bufs.append(p)
            d_in, d_out, d_met = bufs
            check(L.blah2hip_ctx_h2d(ctx, d_in, _ptr(data), data.nbytes))
            if self.n_rates:  # tracks are set: the window sums along them (the index plane is not returned)
                n_out, first = self.process_tracks_dev(d_in, n_cpi, d_out, None, d_met, n_out, w, L.blah2hip_ctx_stream(ctx))
            else:
                n_out, first = self.process_dev(d_in, n_cpi, d_out, d_met, n_out, w, L.blah2hip_ctx_stream(ctx))
            if n_out:
                check(L.blah2hip_ctx_d2h(ctx, _ptr(out), d_out, out.nbytes))
                check(L.blah2hip_ctx_d2h(ctx, _ptr(met), d_met, met.nbytes))
            check(L.blah2hip_ctx_sync(ctx))
        finally:
            for p in bufs:
                L.blah2hip_ctx_free(ctx, p)
            L.blah2hip_ctx_destroy(ctx)
        # (an integrated map is not the engine's device copy: no owner)
        return [Map(None, out[i], amb.delay.copy(), amb.doppler.copy(), float(met[i, 0]), float(met[i, 1]), first + i * self.hop)
                for i in range(n_out)]


class ClutterMapDetector:
    """Clutter-map CFAR on the maps of ``amb`` (blah2hip_cmap_*; no reference counterpart): every cell against
    ``alpha[age]`` times the exponentially weighted average of its own past power, memory ``memory`` CPIs, at false-alarm
    probability ``pfa``.  ``normalise``: the cells are scaled by each CPI's level first (BLAH2HIP_CMAP_NORMALISE).  On its
    own it leaves hit lists like the other detectors'; its exceed plane gates theirs (``gate_dev``): a cell that is bright
    in every CPI is not reported, an echo that moves through cells is.  The average and the age carry over from call to
    call; ``close()`` it before its ``amb``."""

    def __init__(self, amb, pfa, memory, minDelay, minDoppler, normalise=True):
        if not -128 <= int(minDelay) <= 127:  # int8_t in the reference's detector
            raise ValueError("minDelay outside int8 range")
        h = C.c_void_p()
        check(amb._L.blah2hip_cmap_create(amb._h, int(memory), _lib.CMAP_NORMALISE if normalise else 0, C.byref(h)))
        self._h, self._L, self.amb = h, amb._L, amb
        self.pfa, self.memory, self.minDelay, self.minDoppler = float(pfa), int(memory), int(minDelay), float(minDoppler)
        self.normalise = bool(normalise)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.amb, "_h", None):  # (as MapIntegrator.close: never through a closed handle)
                self._L.blah2hip_cmap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self):
        """The threshold table of ``pfa`` onto the device ahead of time (blah2hip_cmap_prepare; blocking)."""
        check(self._L.blah2hip_cmap_prepare(self._h, self.pfa))

    def reset(self):
        """Age 0: the next CPI starts the average anew (host only)."""
        check(self._L.blah2hip_cmap_reset(self._h))

    def age(self):
        """CPIs absorbed since the creation or the last reset."""
        a = C.c_uint64(0)
        check(self._L.blah2hip_cmap_age(self._h, C.byref(a)))
        return a.value

    def background(self):
        """``b``: float32 ``[n_doppler, n_delay]`` (waits for the device)."""
        out = np.empty((self.amb.dims.n_doppler_bins, self.amb.dims.n_delay_bins), dtype=np.float32)
        check(self._L.blah2hip_cmap_read_background(self._h, _ptr(out)))
        return out

    def process_dev(self, n_cpi, d_hits, cap, d_count, d_map=None, d_metrics=None, d_exceed=None, d_level=None, stream=0):
        """Enqueue the next ``n_cpi`` CPIs (blah2hip_cmap_process_dev; raw pointers/ints): hit records into ``d_hits [n_cpi]
        [cap]`` and counts into ``d_count [n_cpi]`` (both None: no list), the uint8 plane ``d_exceed [n_cpi][n_doppler]
        [n_delay]`` and the levels ``d_level [n_cpi]`` when given.  ``d_map`` / ``d_metrics``: None = the engine's own."""
        check(self._L.blah2hip_cmap_process_dev(self._h, d_map, d_metrics, int(n_cpi), self.pfa, self.minDelay, self.minDoppler,
                                                d_hits, int(cap), d_count, d_exceed, d_level, stream))

    def gate_dev(self, d_exceed, n_cpi, d_hits, cap, d_count, d_hits_out, d_count_out, stream=0):
        """Enqueue the gate (blah2hip_cmap_gate_dev): the records of ``d_hits`` whose cell has a non-zero byte in
        ``d_exceed``, in their order, into ``d_hits_out [n_cpi][cap]`` / ``d_count_out [n_cpi]``."""
        check(self._L.blah2hip_cmap_gate_dev(self._h, d_exceed, int(n_cpi), d_hits, int(cap), d_count, d_hits_out, d_count_out,
                                             stream))


class Centroid:
    """src/process/detection/Centroid.h: non-maximum suppression of the CFAR list."""

    def __init__(self, nDelay, nDoppler, resolutionDoppler):
        self.nDelay, self.nDoppler, self.resolutionDoppler = int(nDelay), int(nDoppler), float(resolutionDoppler)

    def process(self, x: Detection) -> Detection:
        L = _lib.load()
        n = x.get_nDetections()
        d, f, s = (np.ascontiguousarray(v, dtype=np.float64) for v in (x.delay, x.doppler, x.snr))
        od, of, os_ = np.zeros(n), np.zeros(n), np.zeros(n)
        k = C.c_uint32(0)
        check(L.blah2hip_centroid(_ptr(d), _ptr(f), _ptr(s), n, self.nDelay, self.nDoppler, self.resolutionDoppler,
                                  _ptr(od), _ptr(of), _ptr(os_), C.byref(k)))
        return Detection(od[:k.value], of[:k.value], os_[:k.value])


class Interpolate:
    """src/process/detection/Interpolate.h: quadratic peak interpolation."""

    def __init__(self, doDelay, doDoppler):
        self.doDelay, self.doDoppler = bool(doDelay), bool(doDoppler)

    def process(self, x: Detection, y: Map) -> Detection:
        L = _lib.load()
        n = x.get_nDetections()
        d, f, s = (np.ascontiguousarray(v, dtype=np.float64) for v in (x.delay, x.doppler, x.snr))
        m = np.ascontiguousarray(y.data, dtype=np.complex64)
        dax = np.ascontiguousarray(y.delay, dtype=np.int32)
        fax = np.ascontiguousarray(y.doppler, dtype=np.float64)
        od, of, os_ = np.zeros(n), np.zeros(n), np.zeros(n)
        k = C.c_uint32(0)
        check(L.blah2hip_interpolate(_ptr(d), _ptr(f), _ptr(s), n, _ptr(m), m.shape[0], m.shape[1], _ptr(dax),
                                     _ptr(fax), float(y.noisePower), int(self.doDelay), int(self.doDoppler),
                                     _ptr(od), _ptr(of), _ptr(os_), C.byref(k)))
        return Detection(od[:k.value], of[:k.value], os_[:k.value])


DET_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("delay", np.float64), ("doppler", np.float64), ("snr", np.float64)])


BEARING_DTYPE = np.dtype([("index", np.int32), ("adaptive", np.int32), ("offset", np.float64), ("power", np.float64),
                          ("coherence", np.float64)])


class DetectionFinisher:
    """:class:`Centroid`, then :class:`Interpolate`, on device-resident hit lists and maps (blah2.cpp:285-287 without the
    host; blah2hip_detect_dev): what the batched chains run behind ``process_dev`` of a detector.  ``doCentroid=False``
    skips the first step; ``doDelay = doDoppler = False`` leaves the list as Centroid returns it."""

    def __init__(self, nDelay, nDoppler, resolutionDoppler, doDelay=True, doDoppler=True, doCentroid=True):
        for name, v in (("nDelay", nDelay), ("nDoppler", nDoppler)):
            if not 0 <= int(v) <= 0xFFFF:  # uint16_t in the reference
                raise ValueError(f"{name} outside uint16 range")
        self.nDelay, self.nDoppler, self.resolutionDoppler = int(nDelay), int(nDoppler), float(resolutionDoppler)
        self.doDelay, self.doDoppler, self.doCentroid = bool(doDelay), bool(doDoppler), bool(doCentroid)

    def process_dev(self, amb, n_cpi, d_hits, cap, d_count, d_out, cap_out, d_count_out, d_map=None, d_metrics=None, stream=0):
        """Enqueue one kernel for n_cpi hit lists (d_hits [n_cpi][cap], d_count [n_cpi], as a detector's ``process_dev``
        wrote them) and their maps (None = the engine's internal buffers): final records (:data:`DET_DTYPE`) into d_out
        [n_cpi][cap_out], their number into d_count_out [n_cpi] (it may exceed cap_out; then cap_out were stored)."""
        check(amb._L.blah2hip_detect_dev(amb._h, d_map, d_metrics, n_cpi, d_hits, cap, d_count, self.nDelay, self.nDoppler,
                                         self.resolutionDoppler, int(self.doCentroid), int(self.doDelay), int(self.doDoppler),
                                         d_out, cap_out, d_count_out, stream))


def dets_to_detection(recs, count, cap_out):
    """One CPI's final records (``blah2hip_det_t``, :data:`DET_DTYPE`; arbitrary order) -> :class:`Detection` in the
    reference's emission order: Centroid and Interpolate keep the detector's row-major order (Centroid.cpp:34-69,
    Interpolate.cpp:35-87), so the records are sorted by the hit they came from."""
    if count > cap_out:
        raise Blah2HipError(_lib.ERR_CAPACITY, f"{count} detections, capacity {cap_out}")
    d = np.asarray(recs[:count])
    d = d[np.lexsort((d["col"], d["row"]))]
    return Detection(d["delay"], d["doppler"], d["snr"])


ATOM_DTYPE = np.dtype([("delay", np.int32), ("reserved", np.int32), ("doppler", np.float64)])


def _atom_pairs(atoms):
    """Atoms as a list of ``(delay int, doppler float)``: from an :data:`ATOM_DTYPE` array or any sequence of pairs."""
    if isinstance(atoms, np.ndarray) and atoms.dtype.names:
        return [(int(d), float(f)) for d, f in zip(atoms["delay"], atoms["doppler"])]
    return [(int(d), float(f)) for d, f in atoms]


def clean_atoms(dets, count, snr_min_db, max_echoes, side_delay, side_doppler, delay_lo, delay_hi, cpi, cap_atoms=_lib.MAX_ATOMS):
    """blah2hip_clean_atoms_dev restated: one CPI's final records (:data:`DET_DTYPE`; ``count`` beyond their number: all of
    them) -> ``(atoms`` :data:`ATOM_DTYPE` ``[n], used [m] int)``.  The records with ``snr >= snr_min_db``, strongest first,
    ties by lower row, then lower col, then lower index, ``max_echoes`` at the most; each becomes the cluster
    ``(rint(delay) + i, doppler + j 0.5 / cpi)``, ``|i| <= side_delay``, ``|j| <= side_doppler``, in the order echo, i, j.
    Members outside ``[delay_lo, delay_hi]`` are dropped; an echo whose remaining members do not fit into ``cap_atoms`` is
    dropped whole, as is one with none left.  ``used``: the indices of the records that gave atoms, in their order."""
    d = np.asarray(dets)[:min(int(count), len(dets))]
    idx = [i for i in range(len(d)) if d["snr"][i] >= snr_min_db]
    idx.sort(key=lambda i: (-d["snr"][i], d["row"][i], d["col"][i], i))
    atoms, used = [], []
    for i in idx[:int(max_echoes)]:
        dc = np.rint(d["delay"][i])
        members = [(int(dc + a), float(d["doppler"][i]) + j * 0.5 / cpi)
                   for a in range(-int(side_delay), int(side_delay) + 1) if delay_lo <= dc + a <= delay_hi
                   for j in range(-int(side_doppler), int(side_doppler) + 1)]
        if members and len(atoms) + len(members) <= cap_atoms:
            atoms += members
            used.append(i)
    out = np.zeros(len(atoms), dtype=ATOM_DTYPE)
    for k, (dl, f) in enumerate(atoms):
        out[k] = (dl, 0, f)
    return out, np.asarray(used, dtype=np.int64)


def clean_replicas(x, atoms, fs):
    """``S [P, N]`` complex128: ``S[p][n] = x[n - d_p] exp(+2j pi f_p n / fs)`` for ``0 <= n - d_p < N``, 0 elsewhere (nothing
    wraps).  A noiseless ``y = S[p]`` peaks in the map cell whose axis values are ``(d_p, f_p)``."""
    x = np.asarray(x, dtype=np.complex128)
    N = x.shape[0]
    n = np.arange(N)
    pairs = _atom_pairs(atoms)
    S = np.zeros((len(pairs), N), dtype=np.complex128)
    for p, (d, f) in enumerate(pairs):
        i = n - d
        ok = (i >= 0) & (i < N)
        S[p, ok] = x[i[ok]] * np.exp(2j * np.pi * ((f * n[ok].astype(np.float64) / fs) % 1.0))
    return S


def clean_fit(x, y, atoms, fs, loading):
    """blah2hip_clean_fit_dev restated in fp64: ``G = S^H S``, ``b = S^H y``, ``(G + loading (tr G / P) I) a = b`` through
    :func:`_cholesky_loaded`.  Returns ``(a [P], ok, G [P, P], b [P])``; ``ok`` is 0 (and ``a`` zero) where a pivot is not
    finite or not above 2^-46 of its loaded diagonal entry (exactly dependent atoms fail without loading), ``a`` is not finite or an atom's Doppler is not finite.  No atoms: ``ok = 1``."""
    pairs = _atom_pairs(atoms)
    P = len(pairs)
    if P and not np.all(np.isfinite([f for _, f in pairs])):
        return np.zeros(P, dtype=np.complex128), 0, np.zeros((P, P), dtype=np.complex128), np.zeros(P, dtype=np.complex128)
    S = clean_replicas(x, pairs, fs)
    G = np.conj(S) @ S.T
    b = np.conj(S) @ np.asarray(y, dtype=np.complex128)
    if P == 0:
        return np.zeros(0, dtype=np.complex128), 1, G, b
    with np.errstate(all="ignore"):
        L, good = _cholesky_loaded(G[None], loading)
        L = L[0]
        v = _forward_solve(L, b)
        a = np.zeros(P, dtype=np.complex128)
        for i in range(P - 1, -1, -1):  # L^H a = v
            s = v[i]
            for p in range(P - 1, i, -1):
                s = s - np.conj(L[p, i]) * a[p]
            a[i] = s / L[i, i].real
        # a pivot must be positive beyond the rounding of its own sum: above 2^-46 of its loaded diagonal entry
        diag = G.diagonal().real + float(loading) * (G.diagonal().real.sum() / P)
        pivots = bool(np.all(L.diagonal().real ** 2 > 2.0 ** -46 * diag))
    ok = int(bool(good[0]) and pivots and bool(np.all(np.isfinite(a))))
    if not ok:
        a = np.zeros(P, dtype=np.complex128)
    return a, ok, G, b


def clean_subtract(x, y, atoms, a, fs):
    """``y - sum_p a_p S[p]`` in fp64 (blah2hip_clean_subtract_dev restated)."""
    y = np.asarray(y, dtype=np.complex128)
    a = np.asarray(a, dtype=np.complex128)
    if a.size == 0:
        return y.copy()
    return y - a @ clean_replicas(x, atoms, fs)


def merge_clean_detections(first, used, second, side_delay, cpi):
    """The two passes' lists of one CPI as one (:data:`DET_DTYPE`): the echoes that were cancelled -- ``first[used]`` --
    then the pass-2 records, less any within ``side_delay + 1`` delay bins and one Doppler bin (``1 / cpi``) of a cancelled
    echo: what is left of it in the second map is its residual, not a new target."""
    first = np.asarray(first)
    second = np.asarray(second)
    gone = first[np.asarray(used, dtype=np.int64)] if len(used) else first[:0]
    keep = np.ones(len(second), dtype=bool)
    for g in gone:
        keep &= ~((np.abs(second["delay"] - g["delay"]) <= side_delay + 1) & (np.abs(second["doppler"] - g["doppler"]) <= 1.0 / cpi))
    return np.concatenate([gone, second[keep]])


class EchoCanceller:
    """Strong-echo cancellation on the samples (blah2hip_clean_*; no reference counterpart): the amplitudes of a list of
    atoms ``(delay, Doppler)`` fitted to the surveillance samples by least squares, their replicas subtracted.  CPIs of
    ``n_samples`` samples at ``fs`` Hz, atom delays in ``[delay_lo, delay_hi]`` (a span of at most 4095).  The ``*_dev``
    methods take raw device pointers and only enqueue."""

    def __init__(self, n_samples, fs, delay_lo, delay_hi, device=0, max_batch=1):
        L = _lib.load()
        h = C.c_void_p()
        check(L.blah2hip_clean_create(int(n_samples), float(fs), int(delay_lo), int(delay_hi), int(device), int(max_batch), C.byref(h)))
        self._h, self._L = h, L
        self.n_samples, self.fs, self.delay_lo, self.delay_hi = int(n_samples), float(fs), int(delay_lo), int(delay_hi)
        self.max_batch = int(max_batch)
        self._last_cap = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.blah2hip_clean_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, option, value):
        check(self._L.blah2hip_clean_set_option(self._h, int(option), int(value)))

    def get_info(self, what):
        v = C.c_int64(0)
        check(self._L.blah2hip_clean_get_info(self._h, int(what), C.byref(v)))
        return v.value

    def atoms_dev(self, amb, d_dets, cap, d_count, n_cpi, snr_min_db, max_echoes, side_delay, side_doppler, d_atoms, cap_atoms,
                  d_atom_count, d_used, stream=0):
        """Enqueue blah2hip_clean_atoms_dev: final records ``d_dets [n_cpi][cap]`` / ``d_count [n_cpi]`` of ``amb`` ->
        ``d_atoms [n_cpi][cap_atoms]`` (:data:`ATOM_DTYPE`), ``d_atom_count [n_cpi]``, ``d_used [n_cpi][cap_atoms]`` int32
        (:func:`clean_atoms`)."""
        check(self._L.blah2hip_clean_atoms_dev(self._h, amb._h, d_dets, int(cap), d_count, int(n_cpi), float(snr_min_db), int(max_echoes),
                                               int(side_delay), int(side_doppler), d_atoms, int(cap_atoms), d_atom_count, d_used, stream))

    def fit_dev(self, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count, loading, d_amp, d_ok, stream=0):
        """Enqueue blah2hip_clean_fit_dev: ``d_amp [n_cpi][cap_atoms]`` (re, im) doubles, ``d_ok [n_cpi]`` int32."""
        check(self._L.blah2hip_clean_fit_dev(self._h, int(fmt), d_x, d_y, int(n_cpi), int(cpi_stride), d_atoms, int(cap_atoms),
                                             d_atom_count, float(loading), d_amp, d_ok, stream))
        self._last_cap = int(cap_atoms)

    def subtract_dev(self, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count, d_amp, d_ok, d_y_out, out_stride,
                     stream=0):
        """Enqueue blah2hip_clean_subtract_dev; ``d_y_out`` may be ``d_y``."""
        check(self._L.blah2hip_clean_subtract_dev(self._h, int(fmt), d_x, d_y, int(n_cpi), int(cpi_stride), d_atoms, int(cap_atoms),
                                                  d_atom_count, d_amp, d_ok, d_y_out, int(out_stride), stream))

    def process_dev(self, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count, loading, d_amp, d_ok, d_y_out,
                    out_stride, stream=0):
        """Enqueue the fit, then the subtraction (blah2hip_clean_process_dev)."""
        check(self._L.blah2hip_clean_process_dev(self._h, int(fmt), d_x, d_y, int(n_cpi), int(cpi_stride), d_atoms, int(cap_atoms),
                                                 d_atom_count, float(loading), d_amp, d_ok, d_y_out, int(out_stride), stream))
        self._last_cap = int(cap_atoms)

    def read_last(self, cpi=0):
        """``(G [cap, cap], b [cap], amp [cap] complex128, ok)`` of CPI ``cpi`` of the last fit, ``cap`` its ``cap_atoms``
        (waits for the device)."""
        cap = self._last_cap
        G, b, a = np.zeros((cap, cap), dtype=np.complex128), np.zeros(cap, dtype=np.complex128), np.zeros(cap, dtype=np.complex128)
        ok = C.c_int32(0)
        check(self._L.blah2hip_clean_read_last(self._h, int(cpi), _ptr(G), _ptr(b), _ptr(a), C.byref(ok)))
        return G, b, a, ok.value

    def set_timing(self, enable=True):
        check(self._L.blah2hip_clean_set_timing(self._h, int(bool(enable))))

    def get_timing(self):
        """``{kernel name: (ms_total, launches)}`` since the last call (waits for the device)."""
        ms = (C.c_double * _lib.CLK_COUNT)()
        n = (C.c_uint32 * _lib.CLK_COUNT)()
        check(self._L.blah2hip_clean_get_timing(self._h, ms, n))
        return {_lib.CLEAN_KERNEL_NAMES[k]: (ms[k], n[k]) for k in range(_lib.CLK_COUNT)}


def _bessel_i0(x):
    """I0 by its series sum_k ((x / 2)^k / k!)^2 (the library's bessel_i0, term for term)."""
    x = np.asarray(x, dtype=np.float64)
    q = 0.25 * x * x
    term, total = np.ones_like(x), np.ones_like(x)
    for k in range(1, 1000):
        term = term * (q / (float(k) * float(k)))
        total = total + term
        if np.all(term < 1e-17 * total):
            break
    return total


def _ddc_sizes(decim, n_taps):
    if int(decim) != decim or not 1 <= decim <= _lib.MAX_DDC_DECIM:
        raise ValueError(f"decimation {decim!r} outside [1, {_lib.MAX_DDC_DECIM}]")
    if int(n_taps) != n_taps or not 1 <= n_taps <= _lib.MAX_DDC_TAPS:
        raise ValueError(f"n_taps {n_taps!r} outside [1, {_lib.MAX_DDC_TAPS}]")
    return int(decim), int(n_taps)


def ddc_design(decim, n_taps, cutoff=0.8, beta=8.0):
    """The NumPy twin of blah2hip_ddc_design: the down-converter's low-pass, a Kaiser-windowed sinc in fp64,
    ``h[t] ~ sinc(2 nu (t - (T-1)/2)) I0(beta sqrt(1 - ((2t - (T-1)) / (T-1))^2))`` with ``nu = cutoff / (2 decim)``,
    normalised to ``sum h = 1`` and symmetric bit for bit."""
    D, T = _ddc_sizes(decim, n_taps)
    if not (0.0 < cutoff <= 1.0):
        raise ValueError("cutoff outside (0, 1]")
    if not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError("beta negative or not finite")
    nu = cutoff / (2.0 * D)
    half = (T + 1) // 2
    k = 2.0 * np.arange(half, dtype=np.float64) - float(T - 1)
    a = math.pi * nu * k
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(a == 0.0, 1.0, np.sin(a) / a)
    rel = k / float(T - 1) if T > 1 else np.zeros(half)
    v = sinc * _bessel_i0(beta * np.sqrt(np.maximum(0.0, 1.0 - rel * rel)))
    h = np.empty(T, dtype=np.float64)
    h[:half] = v
    h[T - half:] = v[::-1]
    s = math.fsum(h)
    if not (math.isfinite(s) and abs(s) > 0.0):
        raise ValueError("the taps sum to zero")
    return h / s


def ddc_taps(h, f, fs):
    """``h[t] exp(+2 pi i f t / fs)`` in fp64 (complex128 ``[T]``): the down-converter's taps of the carrier at offset ``f``
    before their one rounding to fp32 (blah2hip_ddc_read_taps returns the rounded ones)."""
    h = np.asarray(h, dtype=np.float64)
    a = float(f) / float(fs)
    # frac(a t) exactly (integers), about the whole number next to the rounded product, as the library reduces it
    num, den = a.as_integer_ratio()
    k = np.rint(a * np.arange(h.shape[0], dtype=np.float64))
    ang = 2.0 * math.pi * np.array([(num * t - int(k[t]) * den) / den for t in range(h.shape[0])], dtype=np.float64)
    return h * np.cos(ang) + 1j * (h * np.sin(ang))


def _ddc_phasor(r, m0, n):
    """``exp(-2 pi i frac(r m))`` for ``m = m0 .. m0 + n - 1``, the product r m taken exactly (integers)."""
    num, den = float(r).as_integer_ratio()
    fr = np.array([((num * m) % den) / den for m in range(int(m0), int(m0) + int(n))], dtype=np.float64)
    fr = np.where(fr > 0.5, fr - 1.0, fr)
    return np.cos(2.0 * math.pi * fr) - 1j * np.sin(2.0 * math.pi * fr)


def ddc(u, f, fs, D, h, first_sample=0, history=None, g=None, detail=False):
    """The fp64 restatement of the down-converter (blah2hip_ddc_process_dev) in the form the kernel runs:
    ``v[m] = p[m] sum_t g[t] u[m D - t]`` with ``g = fp32(ddc_taps(h, f, fs))``, ``p[m] = exp(-2 pi i frac(r m))``,
    ``r = f D / fs``, ``m`` the absolute output index ``first_sample / D + 0, 1, ...``.

    ``u``: ``[..., n]`` samples (``n`` a multiple of ``D``; leading axes are channels) that start at absolute index
    ``first_sample``; ``history``: the ``T - 1`` samples in front of them (``[..., T - 1]``, zeros when None).  ``g``
    overrides the taps (complex ``[T]``, e.g. the library's read-back).  Returns ``(v [..., n / D], history_out)`` --
    pass ``history_out`` and ``first_sample + n`` on to continue the stream: the pieces equal the uncut result bit for
    bit (the sum runs tap by tap in a fixed order, in real arithmetic) -- and with ``detail`` also
    ``sum_t |g[t]| |u[m D - t]|``, what the contract's bound is made of."""
    D, T = _ddc_sizes(D, np.asarray(h).shape[0] if g is None else np.asarray(g).shape[0])
    u = np.asarray(u, dtype=np.complex128)
    n = u.shape[-1]
    if n % D or int(first_sample) % D:
        raise ValueError("the sample count and first_sample must be multiples of the decimation")
    if g is None:
        g = ddc_taps(h, f, fs).astype(np.complex64)
    g = np.asarray(g).astype(np.complex128)
    lead = u.shape[:-1]
    if history is None:
        history = np.zeros(lead + (T - 1,), dtype=np.complex128)
    history = np.asarray(history, dtype=np.complex128)
    if history.shape != lead + (T - 1,):
        raise ValueError(f"history must have shape {lead + (T - 1,)}")
    ext = np.concatenate([history, u], axis=-1)
    n_out = n // D
    er, ei = np.ascontiguousarray(ext.real), np.ascontiguousarray(ext.imag)
    ar, ai = np.zeros(lead + (n_out,)), np.zeros(lead + (n_out,))
    S = np.zeros(lead + (n_out,))
    mag = np.abs(ext) if detail else None
    for t in range(T - 1, -1, -1):  # u[m D - t] is ext[T - 1 - t + m D]
        sl = slice(T - 1 - t, T - 1 - t + (n_out - 1) * D + 1, D)
        gr, gi = g[t].real, g[t].imag
        ar += gr * er[..., sl]
        ar -= gi * ei[..., sl]
        ai += gr * ei[..., sl]
        ai += gi * er[..., sl]
        if detail:
            S += abs(g[t]) * mag[..., sl]
    p = _ddc_phasor(float(f) * D / float(fs), int(first_sample) // D, n_out)
    v = (ar * p.real - ai * p.imag) + 1j * (ar * p.imag + ai * p.real)
    hist_out = ext[..., ext.shape[-1] - (T - 1):].copy()
    return (v, hist_out, S) if detail else (v, hist_out)


class Channelizer:
    """The digital down-converter on the device (blah2hip_ddc_*; no reference counterpart): up to eight carriers of a
    two-channel stream mixed to zero, low-passed by the real taps ``h`` and decimated by ``decim`` in one pass over the
    samples; :func:`ddc` restates it.  ``offsets``: the carriers' offsets in Hz (``|f| <= fs / 2``).  Calls bring at
    most ``max_rows`` rows of at most ``max_in`` samples; the stream's history is carried from call to call."""

    def __init__(self, fs, decim, h, offsets, max_in, max_rows=1, device=0):
        L = _lib.load()
        hh = np.ascontiguousarray(np.asarray(h, dtype=np.float64).ravel())
        off = np.ascontiguousarray(np.atleast_1d(np.asarray(offsets, dtype=np.float64)).ravel())
        hd = C.c_void_p()
        check(L.blah2hip_ddc_create(float(fs), int(decim), _ptr(hh), int(hh.shape[0]), _ptr(off), int(off.shape[0]), int(max_in),
                                    int(max_rows), int(device), C.byref(hd)))
        self._h, self._L = hd, L
        self.fs, self.decim, self.n_taps, self.offsets = float(fs), int(decim), int(hh.shape[0]), off.copy()
        self.n_carriers, self.max_in, self.max_rows = int(off.shape[0]), int(max_in), int(max_rows)

    def close(self):
        if getattr(self, "_h", None):
            self._L.blah2hip_ddc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, first_sample=0, stream=0):
        """The next call's first sample is absolute sample ``first_sample`` (a multiple of ``decim``); zero history."""
        check(self._L.blah2hip_ddc_reset(self._h, int(first_sample), stream))

    def process_dev(self, fmt, d_x, d_y, n_in, n_rows, in_stride, d_out_x, d_out_y, out_stride, carrier_stride, stream=0):
        """Enqueue blah2hip_ddc_process_dev: ``n_rows`` rows of ``n_in`` samples at ``in_stride`` -> carrier ``c``, row ``r``
        of either output at ``c * carrier_stride + r * out_stride`` complex fp32 values."""
        check(self._L.blah2hip_ddc_process_dev(self._h, int(fmt), d_x, d_y, int(n_in), int(n_rows), int(in_stride), d_out_x, d_out_y,
                                               int(out_stride), int(carrier_stride), stream))

    def taps(self, carrier=0):
        """``g_c`` as the kernel multiplies with it (complex64 ``[n_taps]``, read back from the device)."""
        g = np.zeros(self.n_taps, dtype=np.complex64)
        check(self._L.blah2hip_ddc_read_taps(self._h, int(carrier), _ptr(g)))
        return g

    def get_info(self, what):
        v = C.c_int64(0)
        check(self._L.blah2hip_ddc_get_info(self._h, int(what), C.byref(v)))
        return v.value

    @property
    def tile(self):
        """Outputs per workgroup of this handle."""
        return self.get_info(_lib.DDC_INFO_TILE)

    @property
    def next_sample(self):
        return self.get_info(_lib.DDC_INFO_NEXT_SAMPLE)

    def set_timing(self, enable=True):
        check(self._L.blah2hip_ddc_set_timing(self._h, int(bool(enable))))

    def get_timing(self):
        """``{kernel name: (ms_total, launches)}`` since the last call (waits for the device)."""
        ms = (C.c_double * _lib.DK_COUNT)()
        n = (C.c_uint32 * _lib.DK_COUNT)()
        check(self._L.blah2hip_ddc_get_timing(self._h, ms, n))
        return {_lib.DDC_KERNEL_NAMES[k]: (ms[k], n[k]) for k in range(_lib.DK_COUNT)}


# the fused kernel (range_fir_kernel) convolves a CPI with ONE tap set
_FIR_BLOCKS_REASON = "the fused FIR takes one tap set per CPI: a clutter filter with blocks > 1 runs the two-stage chain"


class WienerHopf:
    """src/process/clutter/WienerHopf.h:68-78: least-squares clutter canceller.

    ``process(x, y)`` returns ``(ok, y_filtered)``; the reference returns the
    bool and replaces the contents of the y FIFO (WienerHopf.cpp:156-160).  When
    the normal equations are not positive definite ``ok`` is False and y is
    returned unchanged (blah2.cpp:270-273 then skips the CPI).

    ``blocks`` > 1: taps per block of ``nSamples / blocks`` samples, the filter's history carried across the block edges
    (blah2hip_clutter_create_ex).  ``process`` then returns the AND of the blocks' flags; ``d_ok``, ``read_last(v)`` and
    ``taps_dev`` count virtual CPIs ``v = cpi * blocks + block``, and ``nBins / fft_len / seg_len`` describe the plan of one
    block.  The range kernel's fused FIR takes one tap set per CPI: ``Ambiguity.set_fir`` refuses such a filter."""

    def __init__(self, delayMin, delayMax, nSamples, device=0, max_batch=1, blocks=1):
        L = _lib.load()
        h = C.c_void_p()
        check(L.blah2hip_clutter_create_ex(delayMin, delayMax, nSamples, int(blocks), device, max_batch, C.byref(h)))
        self._h, self._L = h, L
        self.nSamples = nSamples
        self.blocks = int(blocks)
        self.max_batch = max(1, int(max_batch))
        nb, fl, sl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(L.blah2hip_clutter_get_dims(h, C.byref(nb), C.byref(fl), C.byref(sl)))
        self.nBins, self.fft_len, self.seg_len = nb.value, fl.value, sl.value
        self._corr_grid = 0  # BLAH2HIP_CLUTTER_OPT_CORR_GRID as last set (the library has no read-back; a re-plan returns it to 0)

    def close(self):
        if getattr(self, "_h", None):
            self._L.blah2hip_clutter_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, x, y):
        x = np.ascontiguousarray(x)
        y = np.ascontiguousarray(y)
        if x.shape[0] != self.nSamples or y.shape[0] != self.nSamples:
            # the reference sizes its plans for nSamples (WienerHopf.cpp:7-56) and reads exactly that many
            raise ValueError(f"WienerHopf.process needs {self.nSamples} samples per channel, got {x.shape[0]} and {y.shape[0]}")
        ok = C.c_int(0)
        if x.dtype == np.complex64 and y.dtype == np.complex64:
            out = np.empty(self.nSamples, dtype=np.complex64)
            check(self._L.blah2hip_clutter_process_c32(self._h, _ptr(x), _ptr(y), x.shape[0], _ptr(out), C.byref(ok)))
        else:
            x = x.astype(np.complex128, copy=False)
            y = y.astype(np.complex128, copy=False)
            out = np.empty(self.nSamples, dtype=np.complex128)
            check(self._L.blah2hip_clutter_process_c64(self._h, _ptr(x), _ptr(y), x.shape[0], _ptr(out), C.byref(ok)))
        return (True, out) if ok.value else (False, y.copy())

    def process_dev(self, d_x, d_y, n_cpi, cpi_stride, d_y_out, d_ok=None, stream=0):
        """Enqueue on ``stream``: device complex64 planes, output may alias d_y."""
        check(self._L.blah2hip_clutter_process_dev(self._h, d_x, d_y, n_cpi, cpi_stride, d_y_out, d_ok, stream))

    def process_dev_fmt(self, fmt, d_x, d_y, n_cpi, cpi_stride, d_y_out, out_stride, d_ok=None, stream=0):
        """Enqueue on ``stream`` with the input in format ``fmt`` (FMT_C32 planes, FMT_I8 planes of int8 pairs, or FMT_I16:
        d_x = the interleaved .rspduo buffer); the filtered channel is written as a complex64 plane with ``out_stride`` samples per CPI."""
        check(self._L.blah2hip_clutter_process_dev_fmt(self._h, fmt, d_x, d_y, n_cpi, cpi_stride, d_y_out, out_stride,
                                                       d_ok, stream))

    def estimate_dev_fmt(self, fmt, d_x, d_y, n_cpi, cpi_stride, d_ok=None, stream=0):
        """The filter's correlations, reduction and Toeplitz solve only: the taps stay in the handle (``taps_dev``) for an
        Ambiguity handle that runs the FIR fused into its range kernel (``Ambiguity.set_fir``).  ``fmt``: FMT_C32, FMT_I16
        or FMT_I8, as for ``process_dev_fmt``."""
        check(self._L.blah2hip_clutter_estimate_dev_fmt(self._h, fmt, d_x, d_y, n_cpi, cpi_stride, d_ok, stream))

    def process_multi_dev(self, fmt, d_x, d_ys, n_cpi, cpi_stride, d_youts, out_stride, d_ok=None, stream=0):
        """One reference plane, ``len(d_ys)`` surveillance planes (blah2hip_clutter_process_multi_dev_fmt; raw pointers/ints):
        r, the reference's spectra and the Toeplitz recursion once per CPI, b_k, the taps and the FIR per channel.  ``fmt``:
        FMT_C32 or FMT_I8; ``d_youts``: one complex64 plane per channel, or None to estimate only; ``d_ok``: int32
        [len(d_ys)][n_cpi].  Channel k of CPI c is virtual CPI ``k * n_cpi + c`` of ``d_ok``, ``read_last`` and ``taps_dev``."""
        K = len(d_ys)
        planes = (C.c_void_p * max(1, K))(*[int(p) if p else None for p in d_ys])
        outs = None
        if d_youts is not None:
            if len(d_youts) != K:
                raise ValueError(f"{K} surveillance planes, {len(d_youts)} output planes")
            outs = (C.c_void_p * max(1, K))(*[int(p) if p else None for p in d_youts])
        check(self._L.blah2hip_clutter_process_multi_dev_fmt(self._h, fmt, d_x, planes, K, n_cpi, cpi_stride, outs, out_stride,
                                                             d_ok, stream))

    def taps_dev(self):
        """(device pointer of the taps [max_batch][nBins] complex64, nBins, the filter's first lag)."""
        p, nb, dm = C.c_void_p(), C.c_uint32(), C.c_int32()
        check(self._L.blah2hip_clutter_taps_dev(self._h, C.byref(p), C.byref(nb), C.byref(dm)))
        return p.value, nb.value, dm.value

    def _refresh_dims(self):
        nb, fl, sl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(self._L.blah2hip_clutter_get_dims(self._h, C.byref(nb), C.byref(fl), C.byref(sl)))
        self.nBins, self.fft_len, self.seg_len = nb.value, fl.value, sl.value

    def set_fft_len(self, F):
        """Force the transform length of the correlation / FIR kernels (0 = planner)."""
        self._corr_grid = 0
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_FFT_LEN, int(F)))
        self._refresh_dims()

    def set_fir_carry(self, on):
        """Blocks of F/2 samples with the window overlap carried in registers (filters with nBins - 1 just under F/2); re-plans."""
        self._corr_grid = 0
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_FIR_CARRY, 1 if on else 0))

    def set_corr_form(self, which):
        """'auto' / 'half' / 'window' (``_lib.CLUTTER_CORR_*``)."""
        if isinstance(which, str):
            which = {"auto": _lib.CLUTTER_CORR_AUTO, "half": _lib.CLUTTER_CORR_HALF, "window": _lib.CLUTTER_CORR_WINDOW}[which]
        self._corr_grid = 0
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_CORR, int(which)))
        self._refresh_dims()

    def set_corr_grid(self, grid):
        """Workgroups per CPI of the correlation kernels (tests): 0 = the planner's, else a multiple of 8 from 8 to the
        plan's own count.  Fewer workgroups than segments make each walk several segments.  An option that re-plans
        (``set_fft_len``, ``set_corr_form``, ``set_fir_carry``) returns the handle to 0."""
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_CORR_GRID, int(grid)))
        self._corr_grid = int(grid)

    def last_corr_grid(self):
        """Workgroups per CPI of the last FFT correlation launch (``_lib.CLUTTER_INFO_CORR_GRID``): the planner's at that
        batch or the forced one; 0 before the first launch."""
        v = C.c_int64(0)
        check(self._L.blah2hip_clutter_get_info(self._h, _lib.CLUTTER_INFO_CORR_GRID, C.byref(v)))
        return int(v.value)

    def set_solve_indices_per_thread(self, k):
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_SOLVE_K, int(k)))

    def set_solve_form(self, which, indices_per_lane=0):
        """'auto' / 'stepwise' (one workgroup per CPI, a barrier per order) / 'lookahead' (blocks of 32 orders on several
        workgroups per CPI); ``indices_per_lane`` in {0, 2, 3, 6, 12} fixes the look-ahead form's slice width."""
        if isinstance(which, str):
            which = {"auto": _lib.CLUTTER_SOLVE_AUTO, "stepwise": _lib.CLUTTER_SOLVE_STEPWISE,
                     "lookahead": _lib.CLUTTER_SOLVE_LOOKAHEAD}[which]
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_SOLVE_FORM, int(which)))
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_SOLVE_E, int(indices_per_lane)))

    def set_solve_spin_limit(self, polls):
        """Polls after which a wait of the look-ahead solve gives up (0 = default, about a second).  Tests: a CPI whose
        solve gave up is solved again by the one-workgroup kernel behind it, so the result does not change."""
        check(self._L.blah2hip_clutter_set_option(self._h, _lib.CLUTTER_OPT_SOLVE_SPIN_LIMIT, int(polls)))

    def solve(self, r, b):
        """The filter's Toeplitz solve alone: toeplitz(r) w = b for [n_cpi][nBins] (or [nBins]) complex r, b.
        Returns (ok[n_cpi] bool, w[n_cpi][nBins] complex64)."""
        r = np.atleast_2d(np.asarray(r, dtype=np.complex128))
        b = np.atleast_2d(np.asarray(b, dtype=np.complex128))
        if r.shape != b.shape or r.shape[1] != self.nBins:
            raise ValueError(f"solve needs [n_cpi][{self.nBins}] arrays")
        rb = np.ascontiguousarray(np.stack([r, b], axis=1))
        w = np.empty((r.shape[0], self.nBins), dtype=np.complex64)
        ok = np.zeros(r.shape[0], dtype=np.int32)
        check(self._L.blah2hip_clutter_solve(self._h, _ptr(rb), r.shape[0], _ptr(w), _ptr(ok)))
        return ok.astype(bool), w

    def solve_dev(self, d_rb, n_cpi, d_w, d_ok, stream=0):
        """Enqueue the solve on device arrays: d_rb [n_cpi][2][nBins] complex128, d_w [n_cpi][nBins] complex64, d_ok int32."""
        check(self._L.blah2hip_clutter_solve_dev(self._h, d_rb, n_cpi, d_w, d_ok, stream))

    def solve_info(self):
        """What the last call's Toeplitz solve ran: {'form', 'E' (indices per lane), 'G' (workgroups per CPI), 'fault' (sticky:
        a bounded wait of the look-ahead form ran out at some point), 'retries' (CPIs the gated one-workgroup kernel has solved)}."""
        out = {}
        for name, what in (("form", _lib.CLUTTER_INFO_SOLVE_FORM), ("E", _lib.CLUTTER_INFO_SOLVE_E),
                           ("G", _lib.CLUTTER_INFO_SOLVE_G), ("fault", _lib.CLUTTER_INFO_SOLVE_FAULT),
                           ("retries", _lib.CLUTTER_INFO_SOLVE_RETRIES)):
            v = C.c_int64(0)
            check(self._L.blah2hip_clutter_get_info(self._h, what, C.byref(v)))
            out[name] = int(v.value)
        return out

    def plan_info(self):
        """The plan the next call runs: {'corr' ('half' / 'window'; 'direct': blocks shorter than two filter lengths, fp64 lag sums), 'carry' (the FIR kernel carries the window overlap in
        registers), 'chunks' (chunks of 2048 taps of a long filter, else 0), 'corr_grid' (the forced workgroups per CPI of the
        correlation kernels, 0 = the planner's; ``last_corr_grid`` tells what a launch used)}."""
        out = {}
        for name, what in (("corr", _lib.CLUTTER_INFO_CORR_FORM), ("carry", _lib.CLUTTER_INFO_FIR_CARRY),
                           ("chunks", _lib.CLUTTER_INFO_CHUNKS)):
            v = C.c_int64(0)
            check(self._L.blah2hip_clutter_get_info(self._h, what, C.byref(v)))
            out[name] = int(v.value)
        out["corr"] = {_lib.CLUTTER_CORR_HALF: "half", _lib.CLUTTER_CORR_DIRECT: "direct"}.get(out["corr"], "window")
        out["carry"] = bool(out["carry"])
        out["corr_grid"] = self._corr_grid
        return out

    def read_last(self, cpi=0):
        """(ok, w, r, b) of CPI ``cpi`` of the last call: the nBins filter taps (complex64) and the fp64
        correlations r, b of the normal equations A w = b, A[i][j] = r[i-j] (diagnostics)."""
        w = np.empty(self.nBins, dtype=np.complex64)
        rb = np.empty(2 * self.nBins, dtype=np.complex128)
        ok = C.c_int(0)
        check(self._L.blah2hip_clutter_read_last(self._h, cpi, _ptr(w), _ptr(rb), C.byref(ok)))
        return bool(ok.value), w, rb[:self.nBins].copy(), rb[self.nBins:].copy()

    def set_timing(self, enable=True):
        check(self._L.blah2hip_clutter_set_timing(self._h, 1 if enable else 0))

    def get_timing(self):
        ms = np.zeros(_lib.CK_COUNT, dtype=np.float64)
        cnt = np.zeros(_lib.CK_COUNT, dtype=np.uint32)
        check(self._L.blah2hip_clutter_get_timing(self._h, _ptr(ms), _ptr(cnt)))
        return {name: (float(ms[k]), int(cnt[k])) for k, name in _lib.CLUTTER_KERNEL_NAMES.items()}


class SpectrumAnalyser:
    """src/process/spectrum/SpectrumAnalyser.h:53-62: decimated spectrum of the
    reference channel.  ``process(x)`` returns ``(spectrum, frequency)``: the
    nSpectrum complex values the reference hands to ``IqData::update_spectrum``
    (SpectrumAnalyser.cpp:43-55) and the frequency axis it hands to
    ``update_frequency``, which is always empty (the axis loop runs on a uint32
    that starts at (2^32 - nSpectrum)/2, :64)."""

    def __init__(self, n, bandwidth, device=0, max_batch=1):
        L = _lib.load()
        h = C.c_void_p()
        check(L.blah2hip_spectrum_create(n, float(bandwidth), device, max_batch, C.byref(h)))
        self._h, self._L = h, L
        d, ns, nfft = C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(L.blah2hip_spectrum_get_dims(h, C.byref(d), C.byref(ns), C.byref(nfft)))
        self.decimation, self.nSpectrum, self.nfft = d.value, ns.value, nfft.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.blah2hip_spectrum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, x):
        x = np.ascontiguousarray(x)
        out = np.empty(self.nSpectrum, dtype=np.complex128)
        if x.dtype == np.complex64:
            check(self._L.blah2hip_spectrum_process_c32(self._h, _ptr(x), x.shape[0], _ptr(out)))
        else:
            x = x.astype(np.complex128, copy=False)
            check(self._L.blah2hip_spectrum_process_c64(self._h, _ptr(x), x.shape[0], _ptr(out)))
        return out, np.empty(0, dtype=np.float64)

    def process_dev(self, fmt, d_x, n_cpi, cpi_stride, d_out, stream=0):
        """Enqueue on ``stream``; d_x in format ``fmt`` (FMT_C32, FMT_I16, FMT_F16 or FMT_I8: the reference plane); d_out
        is [n_cpi][nSpectrum] complex128 in HBM."""
        check(self._L.blah2hip_spectrum_process_dev(self._h, fmt, d_x, n_cpi, cpi_stride, d_out, stream))


def deblock_c32_dev(d_raw, block, first, n_samples, n_cpi, d_x, d_y, cpi_stride, stream=0):
    """Enqueue on ``stream``: the x and y planes [n_cpi][cpi_stride] complex64 of a USRP capture's channel-blocked fc32
    bytes at d_raw (blocks of ``block`` samples, x block then y block); CPI i sample j is sample first + i*n_samples + j."""
    check(_lib.load().blah2hip_deblock_c32_dev(d_raw, block, first, n_samples, n_cpi, d_x, d_y, cpi_stride, stream))


def next_hamming(v: int) -> int:
    """src/process/meta/HammingNumber.cpp:38-48."""
    return int(_lib.load().blah2hip_next_hamming(v))
