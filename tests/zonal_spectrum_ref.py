"""numpy restatement of the zonal energy spectrum and MELR of reference scripts/losses.py:16-152 (`ZonalSpectrum`,
`compute_zonal_spectrum`, `MELRCalculator`), the checker of dlwp_benchmark_amd.metrics.ZonalSpectrumMetrics.

PARITY UNPINNED, like oracle/restate/metrics.py: the reference class needs xarray and wandb, which are not available,
and it cannot run as written, so no fixture of it could be recorded.  Its three defects are resolved as follows:
  - `MELRCalculator.__init__` takes no argument but scripts/train.py:96 passes a cfg: the cfg plays no part in the
    metric, the restatement takes none;
  - `self.coords` is never created (losses.py:87): the coordinates it would hold are the sample axis, the latitudes
    (np.linspace(-90, 90, H), losses.py:88, the default here) and the longitudes, which only label the spectrum
    (`lon_spacing_m` feeds the frequency / wavelength coordinates, not the energies);
  - `epsilon` is read at losses.py:113 (the log2 plot columns) before it is assigned at :117: the assignment's value,
    1e-10 (absolute), is the one used, and only the log ratio of :118 is restated.

Definition (float64 throughout): for a field f[..., H, W],
  F[m] = rfft(f, norm="forward")[m], m = 0 .. W/2                                      (losses.py:39)
  P[m] = |F[m]|^2 * (1 if m == 0 else 2)                                               (:40-43, Nyquist doubled too)
  circ_h = cos(lat_h pi / 180) * 2 pi R, R = 1000 (6357 + 6378) / 2                    (:13, :20-23, :69-71)
  E[k, c, m] = mean over samples b and latitudes h of circ_h P[b, k, c, h, m]           (:107-108)
  log_ratio = ln((E_pred + 1e-10) / (E_true + 1e-10)),  MELR = mean over m of log_ratio (:117-121)
"""
import numpy as np

EARTH_RADIUS_M = 1000 * (6357 + 6378) / 2
EPS = 1e-10


def circumference(lats_deg):
    return np.cos(np.asarray(lats_deg, dtype=np.float64) * np.pi / 180) * 2 * np.pi * EARTH_RADIUS_M


def zonal_power(f):
    """P[..., m] of the rows f[..., W] (losses.py:36-44)."""
    fk = np.fft.rfft(np.asarray(f, dtype=np.float64), axis=-1, norm="forward")
    twos = np.concatenate(([1.0], [2.0] * (fk.shape[-1] - 1)))
    return np.real(fk * np.conj(fk)) * twos


def zonal_energy(x, lats_deg=None):
    """E[k, c, m] of a rollout x[B, K, C, H, W]: the sample- and latitude-mean of circ_h P."""
    x = np.asarray(x, dtype=np.float64)
    h = x.shape[-2]
    lats = np.linspace(-90, 90, h) if lats_deg is None else lats_deg
    p = zonal_power(x) * circumference(lats)[:, None]
    return p.mean(axis=0).mean(axis=-2)


def melr(out, target, lats_deg=None):
    """{"energy_pred", "energy_true", "log_ratio": [K, C, W//2 + 1], "melr": [K, C]}."""
    ep, et = zonal_energy(out, lats_deg), zonal_energy(target, lats_deg)
    ratio = np.log((ep + EPS) / (et + EPS))
    return {"energy_pred": ep, "energy_true": et, "log_ratio": ratio, "melr": ratio.mean(axis=-1)}
