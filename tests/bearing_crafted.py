"""Inputs shared by tests/test_bearing_host.py (NumPy only) and tests/test_bearing_gpu.py.

The scene is that of tests/adaptive_crafted.py -- K = 4, a half-wave line array behind a 21 x 111 map, a 40 dB interferer
from -24 degrees on rows 9-11, a 25 dB target from +20 degrees at TARGET_CELL -- plus a SECOND 25 dB target from +20
degrees inside an interferer row, at SHARED_CELL: the cell a passive radar cares about, a target on top of residual direct
path.  It is added before the cells are rounded to complex64, so the statements of adaptive_crafted.scene() are repeated
here with that one more (tests/test_bearing_host.py checks that every other cell is that scene's, bit for bit).

Grids: -88 .. 88 degrees in 1 degree steps for the line array (at half-wave spacing +90 and -90 degrees are the same
steering vector and would tie exactly, so the ends are left out), and 360 points of a uniform circular array for the
wrap cases.
"""
import numpy as np

import adaptive_crafted as A
from blah2_amd import uca_steering, ula_steering
from blah2_amd.process import bearing_powers

K = A.K
SHARED_CELL = (10, 30)          # the second target, inside an interferer row
INTERFERER_CELL = (9, 80)       # the interferer alone
CELLS = (SHARED_CELL, A.TARGET_CELL, INTERFERER_CELL)
LOADING = A.LOADING
ULA_DEG = np.arange(-88.0, 89.0, 1.0)         # 177 points
UCA_DEG = np.arange(0.0, 360.0, 1.0)          # 360 points, a closed circle
UCA_RADIUS = 0.35                             # wavelengths: under half a wavelength between neighbours of four elements


def scene(seed=A.SEED):
    """Channel maps complex64 [K, 1, ND, NC]: adaptive_crafted.scene() with the second target."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((K, A.ND, A.NC)) + 1j * rng.standard_normal((K, A.ND, A.NC))) * np.sqrt(0.5)
    a_i = ula_steering(K, A.SPACING, [A.INTERFERER_DEG])[0]
    a_t = ula_steering(K, A.SPACING, [A.TARGET_DEG])[0]
    phase = np.exp(2j * np.pi * rng.random((len(A.INTERFERER_ROWS), A.NC)))
    z[:, list(A.INTERFERER_ROWS), :] += 10.0 ** (A.INTERFERER_DB / 20.0) * a_i[:, None, None] * phase[None]
    z[:, A.TARGET_CELL[0], A.TARGET_CELL[1]] += 10.0 ** (A.TARGET_DB / 20.0) * a_t
    z[:, SHARED_CELL[0], SHARED_CELL[1]] += 10.0 ** (A.TARGET_DB / 20.0) * a_t
    return z[:, None].astype(np.complex64)


def scene_k(n_surv, n_cpi, seed):
    """The same kind of scene for any channel count and several CPIs (each with its own noise and interferer phases, so their
    covariances differ): complex64 [n_surv, n_cpi, ND, NC].  The interferer is 30 dB, which keeps cond(R_l) under 1e5 at
    eight channels."""
    rng = np.random.default_rng(seed)
    shape = (n_surv, n_cpi, A.ND, A.NC)
    z = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(0.5)
    a_i = ula_steering(n_surv, A.SPACING, [A.INTERFERER_DEG])[0]
    a_t = ula_steering(n_surv, A.SPACING, [A.TARGET_DEG])[0]
    phase = np.exp(2j * np.pi * rng.random((n_cpi, len(A.INTERFERER_ROWS), A.NC)))
    z[:, :, list(A.INTERFERER_ROWS), :] += 31.6 * a_i[:, None, None, None] * phase[None]
    for r, q in (A.TARGET_CELL, SHARED_CELL):
        z[:, :, r, q] += (10.0 ** (A.TARGET_DB / 20.0) * a_t)[:, None]
    return z.astype(np.complex64)


def ula_table(n_surv=K, angles_deg=ULA_DEG):
    """The steering table as the device holds it: complex64 [G, n_surv]."""
    return ula_steering(n_surv, A.SPACING, angles_deg).astype(np.complex64)


def uca_table(n_surv=K, angles_deg=UCA_DEG):
    return uca_steering(n_surv, UCA_RADIUS, angles_deg).astype(np.complex64)


def snapshots(maps, cpi, cells):
    """The K channel cells under (row, col) of ``cells`` in CPI ``cpi``: complex128 [n, K]."""
    rows = np.array([c[0] for c in cells])
    cols = np.array([c[1] for c in cells])
    return np.asarray(maps)[:, cpi, rows, cols].T.astype(np.complex128)


def powers(snap, steer, R=None, loading=0.0):
    """P(g) of blah2_amd.bearing for every snapshot, by numpy.linalg: [n, G] (and t^H t, [n])."""
    s = np.atleast_2d(np.asarray(snap, dtype=np.complex128))
    a = np.asarray(steer, dtype=np.complex128)
    n_surv = s.shape[1]
    L = np.eye(n_surv, dtype=np.complex128)
    if R is not None:
        R = np.asarray(R, dtype=np.complex128)
        L = np.linalg.cholesky(R + loading * (np.trace(R).real / n_surv) * np.eye(n_surv))
    v = np.linalg.solve(L, a.T).T
    t = np.linalg.solve(L, s.T).T
    vv = (np.abs(v) ** 2).sum(axis=1)
    return np.abs(t @ np.conj(v).T) ** 2 / vv[None, :], (np.abs(t) ** 2).sum(axis=1)


def top_two_gap(snap, steer, R=None, loading=0.0):
    """The relative gap between the two largest P(g) of every snapshot, in blah2_amd.bearing's own arithmetic: an index is
    only compared where this is far above rounding."""
    P = np.sort(bearing_powers(snap, steer, R, loading)[0], axis=1)
    return (P[:, -1] - P[:, -2]) / P[:, -1]
