"""Inputs and bounds of the clutter-map tests, shared by test_clutter_map_model.py (CPU) and test_clutter_map_gpu.py: what
the CPU module proves about an input (no cell inside the decision margin, the scene's cells) is what the GPU module runs.

Maps never come from the ambiguity engine: the detector takes any device map.  ``noise`` is complex Gaussian of mean power 1
in complex64; ``levels`` is the factor the detector forms from a map's metrics, ``10 ** (-noisePower / 5)`` with
``noisePower`` the mean of ``10 log10 |z|`` (Map::set_metrics), in fp64.

The bound on b (include/blah2hip.h has the derivation): against the fp64 recursion on the same cells and levels,
``|b - b_fp64| <= (k + 4) 2^-24 U`` with ``k = min(age, T)`` and ``U`` the largest ``u`` the cell has absorbed.  A decision
is safe when ``|u - alpha b| > 2 (k + 4) 2^-24 alpha U'`` with ``U'`` the larger of ``U`` and the cell's own ``u``: twice b's
bound carried through the factor, which also covers the three roundings of ``u`` itself (alpha >= 1 at every pfa below
one half).
"""
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -24

# The cases test_clutter_map_gpu.py compares with the restatement.  21 x 111: an odd cell count, every other plane 8 bytes off
# a 16-byte boundary (and every other exceed plane on an odd address); 48 x 65: a lone last cell; 513 x 411: hundreds of
# workgroups.  T = 2 over 40 CPIs crosses the memory and the table's last entry (age 32) inside one call; 12 CPIs span a
# group of eight and a partial one.  pfa = 1e-2: about one cell in a hundred exceeds, so a wrong factor shows.
Case = namedtuple("Case", "tag nD nC n_cpi T pfa normalise seed")
CASES = [Case("21x111-T8", 21, 111, 12, 8, 1e-2, True, 1), Case("21x112-T3", 21, 112, 9, 3, 1e-2, True, 2),
         Case("48x64-T1", 48, 64, 5, 1, 1e-2, True, 3), Case("48x65-T64", 48, 65, 10, 64, 1e-2, True, 4),
         Case("21x111-T2-40cpi", 21, 111, 40, 2, 1e-2, True, 5), Case("21x111-T8-raw", 21, 111, 9, 8, 1e-2, False, 6),
         Case("513x411-T8", 513, 411, 4, 8, 1e-2, True, 7)]


def case_maps(c):
    """The case's maps: noise whose level moves from CPI to CPI by up to 6 dB (what the normalisation is for)."""
    gain = 1.0 + (np.arange(c.n_cpi) * 5 % 7) / 6.0 if c.normalise else np.ones(c.n_cpi)
    return (noise(c.n_cpi, c.nD, c.nC, c.seed) * gain[:, None, None].astype(np.float32)).astype(np.complex64)


def geom(nD, nC):
    """Ambiguity arguments (the last one ``n_doppler_bins``) of an nD x nC map: tests/cfar_crafted.py's geom."""
    if (nD, nC) == (513, 411):
        return (-10, 400, -256, 256, 2_000_000, 2_000_000, 0)  # BASELINE configs[1]
    n = nD * 1024
    return (-3, nC - 4, -1000, 1000, n, n, nD)


def noise(n_cpi, nD, nC, seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n_cpi, nD, nC)) + 1j * rng.standard_normal((n_cpi, nD, nC))) * np.sqrt(0.5)
    return z.astype(np.complex64)


def noise_power(maps):
    """Map::set_metrics' noisePower per map, fp64: the mean of 10 log10 |z|."""
    m = np.asarray(maps)
    with np.errstate(divide="ignore"):
        return np.array([np.mean(10.0 * np.log10(np.abs(p.astype(np.complex128)))) for p in m])


def metrics(maps):
    """[n_cpi, 2] doubles as the engine writes them: (noisePower, maxPower)."""
    m = np.asarray(maps)
    with np.errstate(divide="ignore"):
        mx = np.array([np.max(10.0 * np.log10(np.abs(p.astype(np.complex128)))) for p in m])
    return np.stack([noise_power(m), mx], axis=1)


def levels(maps):
    return 10.0 ** (-noise_power(maps) / 5.0)


def scene(seed=3, n_cpi=24, nD=21, nC=111, power=30.0):
    """Noise of mean power 1, a fixed discrete of ``power`` at (10, 40) and a target of ``power`` at (4, 20 + g) in CPI g, both
    with a random phase per CPI.  -> (maps, the discrete's cell, the target's cells per CPI)."""
    m = noise(n_cpi, nD, nC, seed).astype(np.complex128)
    rng = np.random.default_rng(seed + 1000)
    ph = rng.uniform(0, 2 * np.pi, (n_cpi, 2))
    a = np.sqrt(power)
    target = []
    for g in range(n_cpi):
        m[g, 10, 40] += a * np.exp(1j * ph[g, 0])
        m[g, 4, 20 + g] += a * np.exp(1j * ph[g, 1])
        target.append((4, 20 + g))
    return m.astype(np.complex64), (10, 40), target


def b_bound(age, memory, umax):
    """The derived bound on |b_device - b_fp64| after ``age`` CPIs."""
    return (min(int(age), int(memory)) + 4) * EPS * np.asarray(umax)


def margin_cells(detail, alpha, memory, age0=0, umax0=None):
    """bool [n_cpi, ...]: the cells whose decision the bound does not settle (they may go either way on the device).  ``detail``:
    clutter_map's third value for a call that started at age ``age0``; ``alpha``: its table; ``umax0``: the largest ``u`` each
    cell had absorbed before the call (clutter_map's ``state["umax"]``; None: nothing, as at age 0)."""
    u, thr = detail["u"], detail["thr"]
    out = np.zeros(u.shape, dtype=bool)
    T = int(memory)
    umax = np.zeros(u.shape[1:]) if umax0 is None else np.array(umax0, dtype=np.float64)
    for c in range(u.shape[0]):
        age = age0 + c
        fin = np.isfinite(u[c])
        uc = np.where(fin, u[c], 0.0)
        if age >= 1:
            al = alpha[min(age, 16 * T)]
            with np.errstate(invalid="ignore"):
                out[c] = fin & (np.abs(uc - thr[c]) <= 2 * (min(age, T) + 4) * EPS * al * np.maximum(umax, uc))
        umax = np.maximum(umax, uc)
    return out


def emulate_f32(maps, lev, memory, age0=0, b0=None):
    """cmap_kernel's arithmetic on b in NumPy: every operation rounded to fp32 where the kernel rounds (the two fused
    multiply-adds are formed in fp64 -- their products are exact there -- and rounded once more, which can differ from a
    true fma in a last bit on rare ties).  -> b float32."""
    m = np.asarray(maps)
    T = int(memory)
    b = np.zeros(m.shape[1:], dtype=np.float32) if b0 is None else np.array(b0, dtype=np.float32)
    for c in range(m.shape[0]):
        age = age0 + c
        re, im = m[c].real.astype(np.float32), m[c].imag.astype(np.float32)
        im2 = (im * im).astype(np.float32)
        p = (re.astype(np.float64) * re.astype(np.float64) + im2.astype(np.float64)).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            u = p if lev is None else (p * np.float32(lev[c])).astype(np.float32)
            fin = np.isfinite(u)
            if age == 0:
                b = np.where(fin, u, np.float32(0)).astype(np.float32)
            else:
                r = np.float32(1.0) / np.float32(min(age + 1, T))
                d = (u - b).astype(np.float32)
                nb = (np.float64(r) * d.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
                b = np.where(fin, nb, b).astype(np.float32)
    return b


def count_variant(u, alpha, memory, variant="right"):
    """Exceeding cells over ages 1 .. n_cpi - 1 of the normalised powers ``u [n_cpi, cells]`` under the definition
    (``right``) or one of four ways to get it wrong: ``frozen`` (the table stops at alpha[T]), ``steady`` (the steady-state
    factor alpha[16 T] at every age), ``nowarm`` (weight 1 / T from the first update on), ``shifted`` (alpha[a + 1] at age
    a)."""
    T = int(memory)
    b = u[0].copy()
    n = 0
    for a in range(1, u.shape[0]):
        idx = {"right": min(a, 16 * T), "frozen": min(a, T), "steady": 16 * T, "nowarm": min(a, 16 * T),
               "shifted": min(a + 1, 16 * T)}[variant]
        n += int(np.count_nonzero(u[a] > alpha[idx] * b))
        k = T if variant == "nowarm" else min(a + 1, T)
        b = b + (u[a] - b) / k
    return n
