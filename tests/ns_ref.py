"""The scheme of dlwp_ns2d_rollout_f32 (csrc/navier_stokes.hip) restated with numpy alone, operation for
operation, in float64 or in float32 (numpy's transforms then run in single precision and every intermediate is stored in it).
The reference tree holds no solver: this file and the closed-form decay of a Taylor-Green vortex are what pins the kernel.

Unit torus, n x n grid, axis 0 the coordinate a = i / n, axis 1 b = j / n; the state is wh = rfft2(w), unnormalised, on the half
plane [n, n / 2 + 1] with integer wavenumbers ka (signed, axis 0) and kb (0 .. n / 2, axis 1)."""
import numpy as np

TWO_PI = 2.0 * np.pi


def _types(dtype):
    dtype = np.dtype(dtype)
    assert dtype in (np.dtype(np.float32), np.dtype(np.float64))
    return dtype, np.dtype(np.complex64 if dtype == np.float32 else np.complex128)


def wavenumbers(n: int):
    """(ka [n, 1], kb [1, n / 2 + 1]) as float64 integers"""
    ka = np.fft.fftfreq(n, d=1.0 / n)[:, None]
    kb = np.fft.rfftfreq(n, d=1.0 / n)[None, :]
    return ka, kb


def tables(n: int):
    """float64 (lap, lapi, mask, nyquist): lap = 4 pi^2 |k|^2, lapi = lap with lapi[0, 0] = 1, mask the 2/3 rule on both
    axes, nyquist the modes |ka| = n / 2 or kb = n / 2"""
    ka, kb = wavenumbers(n)
    lap = 4.0 * np.pi ** 2 * (ka * ka + kb * kb)
    lapi = lap.copy()
    lapi[0, 0] = 1.0
    mask = (np.abs(ka) <= (2.0 / 3.0) * (n / 2)) & (np.abs(kb) <= (2.0 / 3.0) * (n / 2))
    nyquist = (np.abs(ka) == n // 2) | (kb == n // 2)
    return lap, lapi, mask, nyquist


def li2020_forcing(n: int) -> np.ndarray:
    """0.1 (sin 2 pi (a + b) + cos 2 pi (a + b)), float64 [n, n]"""
    t = np.arange(n, dtype=np.float64) / n
    s = TWO_PI * (t[:, None] + t[None, :])
    return 0.1 * (np.sin(s) + np.cos(s))


def grf_amplitude(n: int, tau: float = 7.0, alpha: float = 2.5) -> np.ndarray:
    """float64 [n, n / 2 + 1]: A(k) = n sqrt(2) tau^(alpha - 1) (4 pi^2 |k|^2 + tau^2)^(-alpha / 2), A(0) = 0 -- the covariance of
    the FNO paper's GaussianRF under an unnormalised inverse transform of white noise.  The modes |ka| = n / 2 and kb = n / 2,
    which the solver removes on entry, are zero in the table as well."""
    lap, _, _, nyquist = tables(n)
    amp = n * np.sqrt(2.0) * tau ** (alpha - 1.0) * (lap + tau * tau) ** (-alpha / 2.0)
    amp[0, 0] = 0.0
    amp[nyquist] = 0.0
    return amp


def gaussian_random_field(z: np.ndarray, tau: float = 7.0, alpha: float = 2.5, dtype=np.float64) -> np.ndarray:
    """irfft2(rfft2(z) A) of white noise z [..., n, n]"""
    rt, ct = _types(dtype)
    n = z.shape[-1]
    amp = grf_amplitude(n, tau, alpha).astype(rt)
    zh = np.fft.rfft2(z.astype(rt)).astype(ct)
    return np.fft.irfft2((zh * amp).astype(ct), s=(n, n)).astype(rt)


def solve(w0: np.ndarray, frames: int, substeps: int, dt: float, nu: float, forcing="li2020", filter=None,
          dtype=np.float64) -> np.ndarray:
    """[B, frames, n, n]: frame t is the vorticity after t * substeps sub-steps; frame 0 is w0 filtered and band-limited."""
    rt, ct = _types(dtype)
    w0 = np.asarray(w0)
    assert w0.ndim == 3 and w0.shape[-1] == w0.shape[-2]
    n = w0.shape[-1]
    ka, kb = wavenumbers(n)
    lap, lapi, mask, nyquist = tables(n)
    if isinstance(forcing, str):
        assert forcing == "li2020"
        forcing = li2020_forcing(n)
    dt_, nu_ = rt.type(dt), rt.type(nu)
    lap_r, lapi_r, mask_r = lap.astype(rt), lapi.astype(rt), mask.astype(rt)
    two_pi_i = ct.type(1j * TWO_PI)
    dka, dkb = (two_pi_i * ka.astype(rt)).astype(ct), (two_pi_i * kb.astype(rt)).astype(ct)
    half = (rt.type(0.5) * dt_ * nu_ * lap_r).astype(rt)
    if forcing is None:
        fh = np.zeros((n, n // 2 + 1), dtype=ct)
    else:
        fh = np.fft.rfft2(np.asarray(forcing).astype(rt)).astype(ct)
        fh[nyquist] = 0.0           # as the state's: those modes then stay zero
    wh = np.fft.rfft2(w0.astype(rt)).astype(ct)
    if filter is not None:
        wh = (wh * np.asarray(filter).astype(rt)).astype(ct)
    wh[:, nyquist] = 0.0
    inv = lambda c: np.fft.irfft2(c.astype(ct), s=(n, n)).astype(rt)
    out = np.empty((w0.shape[0], frames, n, n), dtype=rt)
    for t in range(frames):
        out[:, t] = inv(wh)
        if t == frames - 1:
            break
        for _ in range(substeps):
            psi = (wh / lapi_r).astype(ct)
            u, v = inv(dkb * psi), inv(-dka * psi)
            wa, wb = inv(dka * wh), inv(dkb * wh)
            adv = (u * wa + v * wb).astype(rt)
            F = (mask_r * np.fft.rfft2(adv)).astype(ct)
            wh = ((-dt_ * F + dt_ * fh + (rt.type(1.0) - half) * wh) / (rt.type(1.0) + half)).astype(ct)
    return out


def taylor_green(n: int, m: int) -> np.ndarray:
    """cos(2 pi m a) cos(2 pi m b), float64 [n, n]: its advection term vanishes identically"""
    t = np.arange(n, dtype=np.float64) / n
    return np.cos(TWO_PI * m * t)[:, None] * np.cos(TWO_PI * m * t)[None, :]


def taylor_green_decay(m: int, steps: int, dt: float, nu: float) -> float:
    """what the scheme multiplies a Taylor-Green vortex by: ((1 - dt nu lam / 2) / (1 + dt nu lam / 2))^steps, lam = 8 pi^2 m^2"""
    half = 0.5 * dt * nu * 8.0 * np.pi ** 2 * m * m
    return ((1.0 - half) / (1.0 + half)) ** steps


def rel_l2(a: np.ndarray, b: np.ndarray) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
