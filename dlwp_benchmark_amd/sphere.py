"""Host side of the spherical harmonic transforms (csrc/sht.hip): quadrature, Legendre tables, twiddles -- numpy, float64.

Conventions (the specification of ops.sht / ops.isht; they restate torch_harmonics' RealSHT / InverseRealSHT with
norm="ortho", csphase=True from recollection -- PARITY UNPINNED):

  forward   X = 2 pi rfft(x, dim=-1, norm="forward")[..., :mmax]
            c[..., l, m] = sum_k (P[m, l, k] w_k) X[..., k, m]                      complex [..., lmax, mmax]
  inverse   X[..., k, m] = sum_l P[m, l, k] c[..., l, m]
            y = irfft(X, n=nlon, dim=-1, norm="forward")     (imaginary parts of m = 0 and m = nlon / 2 ignored, m >= mmax zero)

P are the orthonormal associated Legendre functions with the Condon-Shortley phase (zero for l < m), w the quadrature
weights of the latitude grid for the integral over cos(theta):  2 pi sum_k w_k P[m, l, k] P[m, l', k] = delta_ll'.
Row 0 of a field is the northernmost latitude (colatitude ascending).

The device never evaluates a transcendental: the kernels read fp32 tables rounded ONCE from the float64 ones made here.
"""
import math
from collections import namedtuple

import numpy as np

from . import lib as _lib

GRIDS = ("legendre-gauss", "equiangular", "equiangular-centred")
MAX_NLAT = 256       # the envelope of the kernels (include/dlwp_hip.h)
MAX_NLON = 512


def quadrature(grid: str, nlat: int):
    """(theta, w): colatitudes in radians, ascending, and the weights of the integral over cos(theta) (they sum to 2).

    "legendre-gauss": the Gauss nodes; exact for polynomials of degree <= 2 nlat - 1, so the Legendre functions are
    orthonormal under it for l + l' <= 2 nlat - 1: every lmax <= nlat.
    "equiangular": Clenshaw-Curtis on theta_j = pi j / (nlat - 1), poles included; exact for degree <= nlat - 1 only, so
    orthonormality holds for l + l' <= nlat - 1.
    "equiangular-centred": the cell-centred grid theta_j = pi (j + 1/2) / nlat (no pole; the lat-lon grids of the reference data,
    healpix.reference_grid) with Fejer's first rule, w_j = (2 / nlat) (1 - 2 sum_{k=1}^{nlat // 2} cos(2 k theta_j) / (4 k^2 - 1)).
    The weights are positive; the rule is exact for degree <= nlat - 1, so, as on "equiangular", orthonormality holds for
    l + l' <= nlat - 1 only: spectra of fields band-limited below nlat / 2 are exact with lmax = nlat / 2, above that they alias."""
    nlat = int(nlat)
    if grid == "lobatto":
        raise NotImplementedError("grid='lobatto' is not supported (no shipped config uses it)")
    if grid not in GRIDS:
        raise _lib.DlwpError(f"unknown grid {grid!r} (one of {GRIDS})")
    if nlat < 2:
        raise _lib.DlwpError(f"nlat = {nlat} must be at least 2")
    if grid == "legendre-gauss":
        x, w = np.polynomial.legendre.leggauss(nlat)       # x ascending: south to north
        return np.arccos(x[::-1]).copy(), w[::-1].copy()
    if grid == "equiangular-centred":
        theta = math.pi * (np.arange(nlat, dtype=np.float64) + 0.5) / nlat
        w = np.ones(nlat, dtype=np.float64)
        for k in range(1, nlat // 2 + 1):
            w -= 2.0 / (4.0 * k * k - 1.0) * np.cos(2.0 * k * theta)
        return theta, w * (2.0 / nlat)
    # Clenshaw-Curtis on theta_j = pi j / (nlat - 1), poles included
    n = nlat - 1
    theta = math.pi * np.arange(nlat, dtype=np.float64) / n
    w = np.ones(nlat, dtype=np.float64)
    for k in range(1, n // 2 + 1):
        b = 1.0 if 2 * k == n else 2.0
        w -= b / (4.0 * k * k - 1.0) * np.cos(2.0 * k * theta)
    c = np.full(nlat, 2.0)
    c[0] = c[-1] = 1.0
    return theta, c * w / n


def latitudes_deg(grid: str, nlat: int) -> np.ndarray:
    """the latitudes of the grid's rows in degrees, 90 - theta: row 0 the northernmost"""
    theta, _ = quadrature(grid, nlat)
    return 90.0 - np.degrees(theta)


def legendre(mmax: int, lmax: int, theta) -> np.ndarray:
    """P[mmax, lmax, nlat]: orthonormal associated Legendre functions at cos(theta), Condon-Shortley phase, zero for l < m.
    The stable three-term recurrence in its orthonormal form (no factorial ever formed)."""
    mmax, lmax = int(mmax), int(lmax)
    x = np.cos(np.asarray(theta, dtype=np.float64))
    n = max(mmax, lmax)
    p = np.zeros((n, n, x.shape[0]), dtype=np.float64)          # [m, l, k]
    p[0, 0] = 1.0 / math.sqrt(4.0 * math.pi)
    for l in range(1, n):
        p[l - 1, l] = math.sqrt(2 * l + 1) * x * p[l - 1, l - 1]
        p[l, l] = np.sqrt((2 * l + 1) * (1.0 - x * x) / (2 * l)) * p[l - 1, l - 1]
    for l in range(2, n):
        for m in range(0, l - 1):
            a = math.sqrt((2 * l - 1) * (2 * l + 1) / ((l - m) * (l + m)))
            b = math.sqrt((l + m - 1) * (l - m - 1) * (2 * l + 1) / ((l - m) * (l + m) * (2 * l - 3)))
            p[m, l] = x * a * p[m, l - 1] - b * p[m, l - 2]
    p = p[:mmax, :lmax].copy()
    p[1::2] *= -1.0
    return p


def check_range(nlat: int, nlon: int, lmax: int, mmax: int):
    if not (2 <= nlat <= MAX_NLAT and 2 <= nlon <= MAX_NLON and nlon % 2 == 0 and 1 <= lmax <= nlat
            and 1 <= mmax <= nlon // 2 + 1):
        raise _lib.DlwpError(f"spherical transform outside the supported range: nlat {nlat} (<= {MAX_NLAT}), nlon {nlon} (even, <= "
                             f"{MAX_NLON}), lmax {lmax} (<= nlat), mmax {mmax} (<= nlon / 2 + 1)")


def tables(grid: str, nlat: int, lmax: int, mmax: int):
    """(wleg, leg) in float64, both [mmax, lmax, nlat]: the forward table P w and the inverse table P."""
    theta, w = quadrature(grid, nlat)
    p = legendre(mmax, lmax, theta)
    return p * w, p


def tables_f32(grid: str, nlat: int, lmax: int, mmax: int):
    """the same two tables rounded once to float32 (what the device holds, in this logical layout)"""
    wleg, leg = tables(grid, nlat, lmax, mmax)
    return wleg.astype(np.float32), leg.astype(np.float32)


def twiddles(nlon: int) -> np.ndarray:
    """[nlon, 2] float64: (cos, -sin)(2 pi t / nlon); the kernels index it by (j m) mod nlon"""
    a = 2.0 * math.pi * np.arange(int(nlon), dtype=np.float64) / int(nlon)
    return np.stack([np.cos(a), -np.sin(a)], axis=-1)


def sht_np(x: np.ndarray, grid: str, lmax: int, mmax: int) -> np.ndarray:
    """the forward transform in float64 on the host, [..., nlat, nlon] -> complex [..., lmax, mmax]"""
    x = np.asarray(x, dtype=np.float64)
    nlat, nlon = x.shape[-2:]
    check_range(nlat, nlon, lmax, mmax)
    wleg, _ = tables(grid, nlat, lmax, mmax)
    xf = 2.0 * math.pi * np.fft.rfft(x, axis=-1, norm="forward")[..., :mmax]
    return np.einsum("mlk,...km->...lm", wleg, xf)


def isht_np(c: np.ndarray, grid: str, nlat: int, nlon: int) -> np.ndarray:
    """the inverse transform in float64 on the host, complex [..., lmax, mmax] -> [..., nlat, nlon]"""
    c = np.asarray(c, dtype=np.complex128)
    lmax, mmax = c.shape[-2:]
    check_range(nlat, nlon, lmax, mmax)
    _, leg = tables(grid, nlat, lmax, mmax)
    xf = np.zeros(c.shape[:-2] + (nlat, nlon // 2 + 1), dtype=np.complex128)
    xf[..., :mmax] = np.einsum("mlk,...lm->...km", leg, c)
    xf[..., 0] = xf[..., 0].real
    xf[..., nlon // 2] = xf[..., nlon // 2].real
    return np.fft.irfft(xf, n=nlon, axis=-1, norm="forward")


# The device tables.  Layouts are the kernels' (csrc/sht.hip), m fastest so that the lanes of a wave, which own consecutive m,
# read consecutive floats:  wleg[k][l][m] = P[m, l, k] w_k,  leg[l][k][m] = P[m, l, k],  tw[t] = (cos, -sin)(2 pi t / nlon).
SphereTables = namedtuple("SphereTables", "wleg leg tw grid nlat nlon lmax mmax")
_device_tables = {}


def device_tables(grid: str, nlat: int, nlon: int, lmax: int, mmax: int, device) -> SphereTables:
    """fp32 tables on `device`, made once per (grid, nlat, nlon, lmax, mmax, device) and kept (a few hundred KB at most)"""
    import torch

    nlat, nlon, lmax, mmax = int(nlat), int(nlon), int(lmax), int(mmax)
    key = (grid, nlat, nlon, lmax, mmax, str(device))
    if key not in _device_tables:
        check_range(nlat, nlon, lmax, mmax)
        wleg, leg = tables_f32(grid, nlat, lmax, mmax)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).contiguous()
        _device_tables[key] = SphereTables(put(wleg.transpose(2, 1, 0)), put(leg.transpose(1, 2, 0)),
                                           put(twiddles(nlon).astype(np.float32)), grid, nlat, nlon, lmax, mmax)
    return _device_tables[key]
