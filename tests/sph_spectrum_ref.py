"""Float64 restatement of the spherical power spectrum sums and scores (dlwp_sph_power_sums_f32, metrics.SphericalSpectrumMetrics;
DESIGN.md section 36) from their definitions -- the reference of tests/test_sph_spectrum_cpu.py and tests/test_sph_spectrum_gpu.py.
Imports nothing from the product; transforms and Legendre tables are those of sht_ref (the derivative route).

For a plane x let c = sht(x), f_m = 1 for m = 0 and 2 m = nlon (where the imaginary part of c is dropped), 2 otherwise:
  power(x)[l] = sum_{m <= min(l, mmax - 1)} f_m |c[l, m]|^2        cross(x, y)[l] = sum_m f_m Re(c_x[l, m] conj c_y[l, m])
  sums [4, K, C, lmax] over b of:  power(out), power(target), power(out - target), cross(out, target)

The cell-centred equiangular grid (theta_j = pi (j + 1/2) / nlat, Fejer's first rule) is not in sht_ref: its weights come here
from the moment equations (a linear solve), not from the closed form the product uses.

`sums_f32` is the float32 restatement that sets the tolerance of the GPU tests: the same fp32 tables as the device, fp32
accumulation, the difference formed in the field domain.
"""
import math

import numpy as np

import sht_ref as R

CENTRED = "equiangular-centred"
MELR_EPS = 1e-10


def quadrature(grid: str, nlat: int):
    """(theta ascending, weights of the integral over cos theta)"""
    if grid != CENTRED:
        return R.quadrature(grid, nlat)
    theta = math.pi * (np.arange(nlat) + 0.5) / nlat
    n = np.arange(nlat)
    a = np.cos(np.outer(n, theta))                                     # T_n(cos theta_j)
    den = 1.0 - n.astype(np.float64) ** 2
    den[1] = 1.0                                                       # n = 1 is odd: its moment is zero
    b = np.where(n % 2 == 0, 2.0 / den, 0.0)                           # integral of T_n over [-1, 1]
    return theta, np.linalg.solve(a, b)


def tables(grid: str, nlat: int, lmax: int, mmax: int):
    """(P [mmax, lmax, nlat], w [nlat]) in float64 by the independent route (lmax, mmax <= 33)"""
    if grid != CENTRED:
        return R.tables(grid, nlat, lmax, mmax)
    theta, w = quadrature(grid, nlat)
    return R.legendre_by_derivatives(mmax, lmax, theta), w


def column_factors(nlon: int, mmax: int) -> np.ndarray:
    f = np.full(mmax, 2.0)
    f[0] = 1.0
    if nlon // 2 < mmax:
        f[nlon // 2] = 1.0
    return f


def _drop_imag(c: np.ndarray, nlon: int) -> np.ndarray:
    c = c.copy()
    c[..., 0] = c[..., 0].real
    if nlon // 2 < c.shape[-1]:
        c[..., nlon // 2] = c[..., nlon // 2].real
    return c


def coefficients(x, p, w) -> np.ndarray:
    """complex128 [..., lmax, mmax] with the imaginary parts of the self-conjugate columns dropped"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return _drop_imag(R.sht(x, p, w).numpy(), x.shape[-1])


def power(x, p, w) -> np.ndarray:
    """[..., lmax]"""
    c = coefficients(x, p, w)
    return (column_factors(np.shape(x)[-1], c.shape[-1]) * (c.real ** 2 + c.imag ** 2)).sum(-1)


def cross(x, y, p, w) -> np.ndarray:
    cx, cy = coefficients(x, p, w), coefficients(y, p, w)
    return (column_factors(np.shape(x)[-1], cx.shape[-1]) * (cx * cy.conj()).real).sum(-1)


def sums(out, target, p, w) -> np.ndarray:
    """float64 [4, K, C, lmax] of out, target [B, K, C, nlat, nlon] (float32 inputs are widened first: the difference is exact)"""
    out, target = np.asarray(out, dtype=np.float64), np.asarray(target, dtype=np.float64)
    return np.stack([power(out, p, w).sum(0), power(target, p, w).sum(0), power(out - target, p, w).sum(0),
                     cross(out, target, p, w).sum(0)])


def sums_f32(out32, target32, wleg32, tw32) -> np.ndarray:
    """the float32 restatement: wleg32 [mmax, lmax, nlat] (P w) and tw32 [nlon, 2] as the device holds them"""
    out32, target32 = np.asarray(out32, dtype=np.float32), np.asarray(target32, dtype=np.float32)
    nlon = out32.shape[-1]
    f = column_factors(nlon, wleg32.shape[0]).astype(np.float32)

    def coeffs(x):
        c = _drop_imag(R.sht_f32(x, wleg32, tw32), nlon)
        return c.real.astype(np.float32), c.imag.astype(np.float32)

    (xr, xi), (yr, yi), (dr, di) = coeffs(out32), coeffs(target32), coeffs(out32 - target32)
    red = lambda t: (f * t).sum(-1, dtype=np.float32).sum(0, dtype=np.float32)
    return np.stack([red(xr * xr + xi * xi), red(yr * yr + yi * yi), red(dr * dr + di * di), red(xr * yr + xi * yi)])


def finalize(s: np.ndarray, n_samples: float) -> dict:
    """the scores of SphericalSpectrumMetrics.finalize from the sums"""
    s = np.asarray(s, dtype=np.float64)
    pw = s[:3] / (4.0 * math.pi * n_samples)
    prod = s[0] * s[1]
    coherence = np.where(prod > 0, s[3] / np.sqrt(np.where(prod > 0, prod, 1.0)), 0.0)
    log_ratio = np.log((pw[0] + MELR_EPS) / (pw[1] + MELR_EPS))
    return {"power_pred": pw[0], "power_true": pw[1], "power_error": pw[2], "coherence": coherence, "log_ratio": log_ratio,
            "selr": log_ratio.mean(-1)}
