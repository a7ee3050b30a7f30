"""On-device evaluation metrics.

`RolloutMetrics` reduces a rollout [B, K, C, H, W] and its targets to latitude-weighted RMSE (and ACC
when a climatology is given) per lead time and variable -- the quantities reference
scripts/evaluate.py:786-821 computes with xarray after copying every trajectory to the host, with the
per-variable de-normalisation of evaluate.py:281-296 folded in as a scale (the means cancel).
Multi-GPU: the [4, K, C] double sums are all-reduced (a few hundred bytes) instead of gathering
trajectories.

`ZonalSpectrumMetrics` reduces the same tensors to zonal energy spectra and the mean energy log ratio (MELR) of
reference scripts/losses.py:16-152, the spectral-blurring score scripts/train.py:434-445 takes of validation rollouts.

Both classes also take HEALPix rollouts [B, K, C, 12, n, n] when they are given the longitudes of the lat-lon grid beside its
latitudes: the reference remaps inits, outputs and targets to lat-lon before every metric (scripts/evaluate.py:298-303,
scripts/train.py:430-441), on the host; here `ops.healpix_to_latlon` does it on the device, a chunk of samples at a time into one
reused workspace, and the sums accumulate through the `*_acc` entry points.
"""
import math
from typing import Optional

import torch

from . import lib as _lib


def latitude_weights(lats_deg: torch.Tensor) -> torch.Tensor:
    """cos(lat_j) / mean_j cos(lat_j)  (evaluate.py:788-790, Eq. (2) of arXiv:2002.00469)."""
    w = torch.cos(torch.deg2rad(lats_deg.double()))
    return (w / w.mean()).float()


DEFAULT_WORKSPACE_BYTES = 256 << 20


class _HealpixInput:
    """What the two metric classes share for HEALPix rollouts [B, K, C, 12, n, n]: the target grid and one workspace per device
    that holds a chunk of samples of `out` and of `target` remapped to lat-lon, within `max_workspace_bytes`."""

    def _init_remap(self, lats_deg, lons_deg, max_workspace_bytes):
        self._lats = torch.as_tensor(lats_deg).detach().double().cpu().reshape(-1).numpy()
        self._lons = None if lons_deg is None else torch.as_tensor(lons_deg).detach().double().cpu().reshape(-1).numpy()
        self.max_workspace_bytes = int(max_workspace_bytes)
        self._remap_ws = {}   # device -> float32 workspace, grown when a shape needs more

    def _require_remap(self, out, target):
        if self._lons is None:
            raise _lib.DlwpError(f"got a {out.dim()}-D rollout {tuple(out.shape)}: a HEALPix rollout [B, K, C, 12, n, n] is remapped "
                                 "to lat-lon only when the metric is built with `lons_deg` (the longitudes of the lat-lon grid)")
        _lib.require_cuda_tensor(out, "out")
        _lib.require_cuda_tensor(target, "target")
        if target.shape != out.shape:
            raise _lib.DlwpError(f"target shape {tuple(target.shape)} != output shape {tuple(out.shape)}")
        if target.device != out.device:
            raise _lib.DlwpError(f"target is on {target.device}, output on {out.device}: both must be on one device")

    def _remapped_chunks(self, out, target):
        """Yields (out, target) as lat-lon [m, K, C, H, W] views of the workspace, m samples at a time, in sample order.  A
        pair is valid until the next one is asked for."""
        from . import ops as _ops

        b, k, c = out.shape[:3]
        h, w = len(self._lats), len(self._lons)
        per = k * c * h * w                                    # floats of one sample of one tensor
        chunk = min(b, self.max_workspace_bytes // (8 * per)) if per else b
        if chunk < 1:
            raise _lib.DlwpError(f"max_workspace_bytes = {self.max_workspace_bytes} does not hold one sample of the rollout and "
                                 f"of the target on the {h}x{w} grid ({8 * per} bytes)")
        key = str(out.device)
        buf = self._remap_ws.get(key)
        if buf is None or buf.numel() < 2 * chunk * per:
            buf = self._remap_ws[key] = torch.empty(2 * chunk * per, dtype=torch.float32, device=out.device)
        for b0 in range(0, b, chunk):
            m = min(chunk, b - b0)
            o = buf[:m * per].view(m, k, c, h, w)
            t = buf[chunk * per:chunk * per + m * per].view(m, k, c, h, w)
            _ops.healpix_to_latlon(out[b0:b0 + m], self._lats, self._lons, out=o)
            _ops.healpix_to_latlon(target[b0:b0 + m], self._lats, self._lons, out=t)
            yield o, t


class RolloutMetrics(_HealpixInput):
    def __init__(self, lats_deg: torch.Tensor, std: Optional[torch.Tensor] = None,
                 climatology: Optional[torch.Tensor] = None, group=None, lons_deg=None,
                 max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        """`lons_deg`: the longitudes of the lat-lon grid; with them `sums` and `__call__` also take HEALPix rollouts
        [B, K, C, 12, n, n], remapped to (lats_deg, lons_deg) on the device in chunks of samples whose lat-lon copies stay within
        `max_workspace_bytes`.  Climatology and latitude weights are lat-lon either way."""
        self._init_remap(lats_deg, lons_deg, max_workspace_bytes)
        self.latw = latitude_weights(lats_deg)
        self.std = std.float() if std is not None else None
        self.clim = climatology.float() if climatology is not None else None
        self.group = group
        self._dev = {}   # device -> (latw, std, clim) copies made once

    def _on(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (self.latw.to(dev).contiguous(),
                              self.std.to(dev).contiguous() if self.std is not None else None,
                              self.clim.to(dev).contiguous() if self.clim is not None else None)
        return self._dev[key]

    def sums(self, out: torch.Tensor, target: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
        """double [4, K, C] sums of this rank's samples (see dlwp_weighted_error_sums_f32).  `into`: a [4, K, C] double tensor
        of running sums the new ones are ADDED to (dlwp_weighted_error_sums_acc_f32: one launch per batch, no zero-fill, no add
        kernel); it is returned.  A HEALPix rollout [B, K, C, 12, n, n] (see `lons_deg`) is remapped chunk by chunk and summed
        into zero-initialised (or `into`) sums."""
        if isinstance(out, torch.Tensor) and out.dim() == 6:
            self._require_remap(out, target)
            sums = into if into is not None else torch.zeros(4, out.shape[1], out.shape[2], dtype=torch.float64, device=out.device)
            for o, t in self._remapped_chunks(out, target):
                self.sums(o, t, into=sums)
            return sums
        _lib.require_cuda_tensor(out, "out")
        _lib.require_cuda_tensor(target, "target")
        out, target = out.contiguous(), target.contiguous()
        b, k, c, h, w = out.shape
        if target.shape != out.shape:
            raise _lib.DlwpError(f"target shape {tuple(target.shape)} != output shape {tuple(out.shape)}")
        dev = out.device
        latw, std, clim = self._on(dev)
        if into is not None:
            if not isinstance(into, torch.Tensor) or not into.is_cuda:
                raise _lib.DlwpError("running sums must be a tensor on an MI355X device")
            if tuple(into.shape) != (4, k, c) or into.dtype != torch.float64 or not into.is_contiguous() or into.device != dev:
                raise _lib.DlwpError(f"running sums must be a contiguous double [4, {k}, {c}] tensor on {dev}")
        sums = into if into is not None else torch.empty(4, k, c, dtype=torch.float64, device=dev)
        _lib.launch("dlwp_weighted_error_sums_acc_f32" if into is not None else "dlwp_weighted_error_sums_f32", dev, out, target,
                    clim, latw, std, sums, b, k, c, h, w)
        return sums

    def __call__(self, out: torch.Tensor, target: torch.Tensor, world_size: int = 1):
        """Returns {"rmse": [K, C], "acc": [K, C] or None} over ALL ranks' samples."""
        cells = len(self._lats) * len(self._lons) if out.dim() == 6 and self._lons is not None else out.shape[-2] * out.shape[-1]
        return self.finalize(self.sums(out, target), float(out.shape[0]), cells, world_size)

    def finalize(self, s: torch.Tensor, n_samples: float, cells: int, world_size: int = 1):
        """Scores from accumulated sums: `s` = this rank's [4, K, C] sums (of one batch, or ADDED UP over many -- the
        reference accumulates squared errors over the whole evaluation before taking the root, evaluate.py:786-821),
        n_samples = how many samples went into them, cells = H * W.  With world_size > 1 ONE all-reduce moves the sums
        and the sample count (shards may differ in size): the only collective of a sharded evaluation."""
        if world_size > 1:
            import torch.distributed as dist

            host = dist.get_backend(self.group) != "nccl"
            dev = s.device
            buf = torch.empty(s.numel() + 1, dtype=torch.float64, device=dev)
            buf[:-1].copy_(s.flatten())
            buf[-1:].fill_(n_samples)   # the count travels with the sums
            if host:
                buf = buf.cpu()
            dist.all_reduce(buf, group=self.group)
            buf = buf.to(dev)
            s, n_samples = buf[:-1].view_as(s), buf[-1:]
        count = n_samples * cells
        rmse = torch.sqrt(s[0] / count)
        acc = s[1] / torch.sqrt(s[2] * s[3]) if self.clim is not None else None
        return {"rmse": rmse, "acc": acc}


EARTH_RADIUS_M = 1000 * (6357 + 6378) / 2   # reference scripts/losses.py:13
MELR_EPS = 1e-10                            # losses.py:117, absolute


def circumference_weights(lats_deg: torch.Tensor) -> torch.Tensor:
    """cos(lat_h) * 2 pi R in float64: the length of each circle of latitude (losses.py:20-23)."""
    return torch.cos(lats_deg.double() * (math.pi / 180)) * (2 * math.pi * EARTH_RADIUS_M)


class ZonalSpectrumMetrics(_HealpixInput):
    """Zonal energy spectra of a rollout [B, K, C, H, W] and its targets, and their mean energy log ratio (reference
    scripts/losses.py:16-152, `ZonalSpectrum` + `MELRCalculator`), reduced on the device (dlwp_zonal_power_sums_f32).

    E[k, c, m] = mean over samples b and latitudes h of circ_h P[b, k, c, h, m], P = |rfft(norm="forward")|^2 along the
    W longitudes with every m > 0 doubled; log_ratio = ln((E_pred + 1e-10) / (E_true + 1e-10)); MELR = its mean over
    m = 0 .. W/2.  The reference places its latitudes at np.linspace(-90, 90, H) (losses.py:88): pass
    `torch.linspace(-90, 90, H)` as `lats_deg` to reproduce scripts/train.py:434-445, or the grid's own cell centres.
    Fields are scored as given (the reference scores normalised fields).  W must be a power of two from 32 to 512.
    With `lons_deg` (the W longitudes of the lat-lon grid) HEALPix rollouts [B, K, C, 12, n, n] are taken too: they are remapped
    to (lats_deg, lons_deg) on the device as scripts/train.py:430-441 remaps them on the host, in chunks of samples whose lat-lon
    copies stay within `max_workspace_bytes`; without it they are refused."""

    def __init__(self, lats_deg: torch.Tensor, group=None, lons_deg=None, max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        self._init_remap(lats_deg, lons_deg, max_workspace_bytes)
        self.circ = circumference_weights(torch.as_tensor(lats_deg))
        self.height = int(self.circ.numel())
        self.group = group
        self._dev = {}   # device -> circumference weights on it
        self._ws = {}    # device -> workspaces, the last one the largest and the one in use

    def _on(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = self.circ.to(dev).contiguous()
        return self._dev[key]

    def _workspace(self, dev, shape):
        """One workspace per device, shared by every shape: a shape that needs more replaces it by one at least twice as large.
        The replaced ones stay allocated because a recorded step (sharding.CapturedStep) keeps the address it was recorded
        with; with the doubling they add up to less than the one in use."""
        n = max(int(_lib.load().dlwp_zonal_power_workspace_bytes(*shape)), 8)
        bufs = self._ws.setdefault(str(dev), [])
        if not bufs or bufs[-1].numel() < n:
            bufs.append(torch.empty(max(n, 2 * bufs[-1].numel()) if bufs else n, dtype=torch.uint8, device=dev))
        return bufs[-1]

    def sums(self, out: torch.Tensor, target: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
        """double [2, K, C, W//2 + 1]: 0 = sum over this rank's samples and latitudes of circ_h P(out), 1 = of P(target)
        (dlwp_zonal_power_sums_f32).  `into`: a [2, K, C, W//2 + 1] double tensor of running sums the new ones are ADDED to
        (dlwp_zonal_power_sums_acc_f32); it is returned.  A HEALPix rollout [B, K, C, 12, n, n] (see `lons_deg`) is remapped chunk
        by chunk and summed into zero-initialised (or `into`) sums."""
        _lib.require_cuda_tensor(out, "out")
        _lib.require_cuda_tensor(target, "target")
        if out.dim() == 6 and self._lons is not None:
            self._require_remap(out, target)
            sums = into if into is not None else torch.zeros(2, out.shape[1], out.shape[2], len(self._lons) // 2 + 1,
                                                             dtype=torch.float64, device=out.device)
            for o, t in self._remapped_chunks(out, target):
                self.sums(o, t, into=sums)
            return sums
        if out.dim() != 5:
            raise _lib.DlwpError(f"zonal spectrum: expected a lat-lon rollout [B, K, C, H, W], got {out.dim()}-D shape "
                                 f"{tuple(out.shape)} (a HEALPix rollout [B, K, C, 12, n, n] is remapped to lat-lon only when the "
                                 "metric is built with `lons_deg`)")
        if target.shape != out.shape:
            raise _lib.DlwpError(f"target shape {tuple(target.shape)} != output shape {tuple(out.shape)}")
        if target.device != out.device:
            raise _lib.DlwpError(f"target is on {target.device}, output on {out.device}: both must be on one device")
        b, k, c, h, w = out.shape
        if h != self.height:
            raise _lib.DlwpError(f"zonal spectrum: {h} latitudes in the rollout, {self.height} given to the metric")
        out, target = out.contiguous(), target.contiguous()
        dev = out.device
        nb = w // 2 + 1
        if into is not None:
            if not isinstance(into, torch.Tensor) or not into.is_cuda:
                raise _lib.DlwpError("running sums must be a tensor on an MI355X device")
            if tuple(into.shape) != (2, k, c, nb) or into.dtype != torch.float64 or not into.is_contiguous() or into.device != dev:
                raise _lib.DlwpError(f"running sums must be a contiguous double [2, {k}, {c}, {nb}] tensor on {dev}")
        circ = self._on(dev)
        ws = self._workspace(dev, (b, k, c, h, w))
        sums = into if into is not None else torch.empty(2, k, c, nb, dtype=torch.float64, device=dev)
        _lib.launch("dlwp_zonal_power_sums_acc_f32" if into is not None else "dlwp_zonal_power_sums_f32", dev, out, target, circ,
                    sums, b, k, c, h, w, ws, ws.numel())
        return sums

    def __call__(self, out: torch.Tensor, target: torch.Tensor, world_size: int = 1):
        """Energies, log ratio and MELR over ALL ranks' samples (see finalize)."""
        return self.finalize(self.sums(out, target), float(out.shape[0]), world_size)

    def finalize(self, s: torch.Tensor, n_samples: float, world_size: int = 1):
        """Scores from accumulated sums: `s` = this rank's [2, K, C, W//2 + 1] sums (of one batch or added up over many),
        n_samples = how many samples went into them.  With world_size > 1 ONE all-reduce moves the sums and the sample
        count (shards may differ in size).  Returns {"energy_pred", "energy_true", "log_ratio": [K, C, W//2 + 1],
        "melr": [K, C]} in float64."""
        if world_size > 1:
            import torch.distributed as dist

            host = dist.get_backend(self.group) != "nccl"
            dev = s.device
            buf = torch.empty(s.numel() + 1, dtype=torch.float64, device=dev)
            buf[:-1].copy_(s.flatten())
            buf[-1:].fill_(n_samples)   # the count travels with the sums
            if host:
                buf = buf.cpu()
            dist.all_reduce(buf, group=self.group)
            buf = buf.to(dev)
            s, n_samples = buf[:-1].view_as(s), buf[-1:]
        energy = s / (n_samples * self.height)
        log_ratio = torch.log((energy[0] + MELR_EPS) / (energy[1] + MELR_EPS))
        return {"energy_pred": energy[0], "energy_true": energy[1], "log_ratio": log_ratio, "melr": log_ratio.mean(dim=-1)}
