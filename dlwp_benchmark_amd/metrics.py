"""On-device evaluation metrics.

`RolloutMetrics` reduces a rollout [B, K, C, H, W] and its targets to latitude-weighted RMSE (and ACC
when a climatology is given) per lead time and variable -- the quantities reference
scripts/evaluate.py:786-821 computes with xarray after copying every trajectory to the host, with the
per-variable de-normalisation of evaluate.py:281-296 folded in as a scale (the means cancel).
Multi-GPU: the [4, K, C] double sums are all-reduced (a few hundred bytes) instead of gathering
trajectories.

`ZonalSpectrumMetrics` reduces the same tensors to zonal energy spectra and the mean energy log ratio (MELR) of
reference scripts/losses.py:16-152, the spectral-blurring score scripts/train.py:434-445 takes of validation rollouts.

`SoundnessMetrics` streams a rollout of any length chunk by chunk into the sums over lead time behind the physical-soundness
scores of scripts/evaluate.py:832-872 (RMSE of the time-and-longitude mean per latitude band, RMSE of the mean field of lead days
334-365); `soundness_scores` turns the sums into the scores in plain torch.

`EnsembleMetrics` scores ensemble forecasts of the diffusion backbones [M, B, K, C, H, W] (rollout.ensemble_chunks /
ensemble_forecast): RMSE of the ensemble mean, spread, spread / skill, CRPS and the rank histogram, streamed chunk by chunk
through dlwp_ensemble_sums_acc_f32 (csrc/ensemble_scores.hip).  The reference has only a commented sketch of it
(scripts/train.py:352-371): PARITY UNPINNED.

`SphericalSpectrumMetrics` reduces a rollout and its targets to the power per total wavenumber l of forecast, truth and error
and to their spectral coherence, through one fused spherical-harmonic transform-and-reduce kernel (csrc/sph_power.hip; DESIGN.md
section 36).  The reference has no spherical spectrum: PARITY UNPINNED.

The five classes differ in their kernel and their scores; everything around them is `_Scorer`'s, defined once: the checks on an
(out, target) pair, the device copies of host constants, the kernel workspace, the cross-rank all-reduce, and HEALPix input.
All five take HEALPix rollouts [B, K, C, 12, n, n] when they are given the longitudes of the lat-lon grid beside its latitudes:
the reference remaps inits, outputs and targets to lat-lon before every metric (scripts/evaluate.py:298-303,
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


class _Scorer:
    """What the metric classes share.  `constants`: host tensors (or None) the kernel reads, copied to a device on first use.
    `lons_deg`: the longitudes of the lat-lon grid; with them HEALPix input is remapped to (lats_deg, lons_deg) on the device in
    chunks of samples whose lat-lon copies stay within `max_workspace_bytes`, without them it is refused."""

    def __init__(self, lats_deg, lons_deg, max_workspace_bytes, group, constants=()):
        self._lats = torch.as_tensor(lats_deg).detach().double().cpu().reshape(-1).numpy()
        self._lons = None if lons_deg is None else torch.as_tensor(lons_deg).detach().double().cpu().reshape(-1).numpy()
        self.max_workspace_bytes = int(max_workspace_bytes)
        self.group = group
        self._constants = tuple(constants)
        self._dev = {}        # device -> the constants on it
        self._ws = {}         # device -> kernel workspaces, the last one the largest and the one in use
        self._remap_ws = {}   # device -> float32 remap workspace, replaced when a shape needs more

    def _on(self, dev):
        """The constants on `dev`, in the order given to __init__ (None stays None), copied once."""
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(dev).contiguous() if t is not None else None for t in self._constants)
        return self._dev[key]

    def _workspace(self, dev, nbytes):
        """One kernel workspace per device, shared by every shape and kept when it grows (lib.kept_workspace)."""
        return _lib.kept_workspace(self._ws, nbytes, dev)

    def _pair_shape(self, out, target, name="out", lead=""):
        """(B, K, C, H, W) of two tensors of one shape: lat-lon [B, K, C, H, W], or HEALPix [B, K, C, 12, n, n] when the metric
        has longitudes, with the H, W of its grid.  Looks at no device, so a caller may put host-side checks of its own next.
        `name`, `lead`: what the caller's argument is called and the dimensions it has in front of these (EnsembleMetrics
        passes a member of `ens` and "M, "), for the messages."""
        if not isinstance(out, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise _lib.DlwpError(f"{name} and target must be tensors")
        if target.shape != out.shape:
            raise _lib.DlwpError(f"target shape {tuple(target.shape)} != {'member' if lead else 'output'} shape "
                                 f"{tuple(out.shape)}")
        if out.dim() == 5:
            return tuple(out.shape)
        if out.dim() == 6 and self._lons is not None:
            return tuple(out.shape[:3]) + (len(self._lats), len(self._lons))
        raise _lib.DlwpError(f"expected lat-lon `{name}` [{lead}B, K, C, H, W], got {'members of ' if lead else ''}{out.dim()}-D "
                             f"shape {tuple(out.shape)}: HEALPix input [{lead}B, K, C, 12, n, n] is remapped to lat-lon only when "
                             "the metric is built with `lons_deg` (the longitudes of the lat-lon grid)")

    @staticmethod
    def _pair_device(out, target, name="out"):
        """The one MI355X device both float32 tensors are on."""
        _lib.require_cuda_tensor(out, name)
        _lib.require_cuda_tensor(target, "target")
        if target.device != out.device:
            raise _lib.DlwpError(f"target is on {target.device}, {name} on {out.device}: both must be on one device")
        return out.device

    def _check_pair(self, out, target, name="out", lead=""):
        shape = self._pair_shape(out, target, name, lead)
        self._pair_device(out, target, name)
        return shape

    def _remapped_chunks(self, *tensors):
        """Yields the sample-major HEALPix tensors [B, K, C, 12, n, n] as lat-lon [m, K, C, H, W] views of the workspace, one per
        tensor in the order given, m samples at a time in sample order: max_workspace_bytes // (4 x tensors x floats per sample)
        of them, every tensor's share of a sample in the same chunk.  The views are valid until the next ones are asked for.
        Layout, which callers may rely on: the views of one chunk lie one fixed distance apart in the workspace, in the order
        given, so the first M of them are one block of M planes `views[1].storage_offset() - views[0].storage_offset()` floats
        apart (what dlwp_ensemble_sums_acc_f32 takes as its members).
        The workspace is exactly as large as the shape needs and is REPLACED by a larger one when a later shape needs more --
        `max_workspace_bytes` bounds it, which doubling would not respect -- so a recorded step (sharding.CapturedStep), which
        keeps the address it was recorded with, must not see a growing HEALPix shape."""
        from . import ops as _ops

        b, k, c = tensors[0].shape[:3]
        h, w = len(self._lats), len(self._lons)
        n = len(tensors)
        per = k * c * h * w                                    # floats of one sample of one tensor
        chunk = min(b, self.max_workspace_bytes // (4 * n * per)) if per else b
        if chunk < 1:
            raise _lib.DlwpError(f"max_workspace_bytes = {self.max_workspace_bytes} does not hold one sample of the {n} tensors "
                                 f"on the {h}x{w} grid ({4 * n * per} bytes)")
        dev = tensors[0].device
        buf = self._remap_ws.get(str(dev))
        if buf is None or buf.numel() < n * chunk * per:
            buf = self._remap_ws[str(dev)] = torch.empty(n * chunk * per, dtype=torch.float32, device=dev)
        for b0 in range(0, b, chunk):
            m = min(chunk, b - b0)
            views = [buf[i * chunk * per:i * chunk * per + m * per].view(m, k, c, h, w) for i in range(n)]
            for x, v in zip(tensors, views):
                _ops.healpix_to_latlon(x[b0:b0 + m], self._lats, self._lons, out=v)
            yield views

    def _healpix_sums(self, out, target, into, shape):
        """`sums` of a HEALPix pair: remapped chunk by chunk and summed into `into`, or into zero-initialised sums of `shape`."""
        sums = into if into is not None else torch.zeros(shape, dtype=torch.float64, device=out.device)
        for o, t in self._remapped_chunks(out, target):
            self.sums(o, t, into=sums)
        return sums

    def _reduce(self, buf):
        """A 1-D double tensor summed over the ranks of `self.group`, on the device it came from: it travels through the host
        unless the group's backend is nccl."""
        import torch.distributed as dist

        dev = buf.device
        if dist.get_backend(self.group) != "nccl":
            buf = buf.cpu()
        dist.all_reduce(buf, group=self.group)
        return buf.to(dev)

    def _reduce_sums(self, s, n_samples):
        """(sums, sample count) over all ranks in ONE all-reduce: the count travels with the sums (shards may differ in size)."""
        buf = torch.empty(s.numel() + 1, dtype=torch.float64, device=s.device)
        buf[:-1].copy_(s.flatten())
        buf[-1:].fill_(n_samples)
        buf = self._reduce(buf)
        return buf[:-1].view_as(s), buf[-1:]


class RolloutMetrics(_Scorer):
    def __init__(self, lats_deg: torch.Tensor, std: Optional[torch.Tensor] = None,
                 climatology: Optional[torch.Tensor] = None, group=None, lons_deg=None,
                 max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        """`lons_deg`: the longitudes of the lat-lon grid; with them `sums` and `__call__` also take HEALPix rollouts
        [B, K, C, 12, n, n], remapped to (lats_deg, lons_deg) on the device in chunks of samples whose lat-lon copies stay within
        `max_workspace_bytes`.  Climatology and latitude weights are lat-lon either way."""
        self.latw = latitude_weights(lats_deg)
        self.std = std.float() if std is not None else None
        self.clim = climatology.float() if climatology is not None else None
        super().__init__(lats_deg, lons_deg, max_workspace_bytes, group, (self.latw, self.std, self.clim))

    def sums(self, out: torch.Tensor, target: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
        """double [4, K, C] sums of this rank's samples (see dlwp_weighted_error_sums_f32).  `into`: a [4, K, C] double tensor
        of running sums the new ones are ADDED to (dlwp_weighted_error_sums_acc_f32: one launch per batch, no zero-fill, no add
        kernel); it is returned.  A HEALPix rollout [B, K, C, 12, n, n] (see `lons_deg`) is remapped chunk by chunk and summed
        into zero-initialised (or `into`) sums."""
        b, k, c, h, w = self._check_pair(out, target)
        if out.dim() == 6:
            return self._healpix_sums(out, target, into, (4, k, c))
        out, target = out.contiguous(), target.contiguous()
        dev = out.device
        latw, std, clim = self._on(dev)
        if into is not None:
            _lib.require_running_sums(into, (4, k, c), dev)
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
            s, n_samples = self._reduce_sums(s, n_samples)
        count = n_samples * cells
        rmse = torch.sqrt(s[0] / count)
        acc = s[1] / torch.sqrt(s[2] * s[3]) if self.clim is not None else None
        return {"rmse": rmse, "acc": acc}


DEFAULT_BANDS = {"global": None, "trade_winds": [(-20, -10), (10, 20)], "south_westerlies": [(-55, -45)]}   # evaluate.py:839-857
_NS_PER_DAY = 86400 * 10 ** 9


def window_steps(step_days: float, window_days=(334.0, 365.0)):
    """The rollout steps [first, last + 1) whose lead time lies in the window: step k (0-based) has lead time (k + 1) step_days
    (evaluate.py:346-347) and belongs when window_days[0] <= lead <= window_days[1], both ends included as in xarray's label
    slice (evaluate.py:868-869).  Whole nanoseconds, as Timedelta labels compare; (0, 0) when no step belongs."""
    sd, lo, hi = (int(round(float(v) * _NS_PER_DAY)) for v in (step_days, window_days[0], window_days[1]))
    if sd <= 0:
        raise _lib.DlwpError(f"step_days must be positive, got {step_days}")
    first, end = max(-(-lo // sd) - 1, 0), hi // sd
    return (first, end) if end > first else (0, 0)


def band_rows(lats_deg: torch.Tensor, intervals) -> torch.Tensor:
    """bool [H]: the latitude rows in any of the closed intervals [(lo, hi), ...] (`.sel(lat=slice(lo, hi))` and the merge of
    evaluate.py:847-856); None = every row."""
    lats = torch.as_tensor(lats_deg).detach().double().cpu().reshape(-1)
    if intervals is None:
        return torch.ones(lats.numel(), dtype=torch.bool)
    rows = torch.zeros(lats.numel(), dtype=torch.bool)
    for lo, hi in intervals:
        rows |= (lats >= lo) & (lats <= hi)
    return rows


def soundness_scores(zonal: torch.Tensor, window: Optional[torch.Tensor], steps: int, n_window_steps: int, width: int, lats_deg,
                     bands=None, std: Optional[torch.Tensor] = None, all_reduce=None):
    """The physical-soundness scores of evaluate.py:832-872 from accumulated sums (dlwp_climate_sums_acc_f32), in plain torch
    on whatever device the sums are on (CPU included).
      zonal [2, B, C, H] double: sums over `steps` steps and `width` longitudes (0 = rollout, 1 = truth)
      window [2, B, C, H, W] double or None: sums over the `n_window_steps` steps of the lead-time window
    A = zonal / (steps width) is the mean over ("time", "lon") (:839-840), M = window / n_window_steps the window's mean over
    "time" (:868-869).  rmse[band][c] = sqrt(mean over samples and the band's rows of (std_c (A_pred - A_true))^2) (:841-857),
    rmse_window[c] = sqrt(mean over samples, rows and columns of (std_c (M_pred - M_true))^2) (:870); no latitude weights (the
    reference applies none here).  A band without a row gives NaN, as an empty xarray mean does.  `all_reduce`: a callable
    that sums a 1-D double tensor over the ranks of a sharded evaluation and returns it -- the squares and the sample count
    go through it in ONE call."""
    bands = DEFAULT_BANDS if bands is None else bands
    dev = zonal.device
    _, b, c, h = zonal.shape
    scale = torch.ones(c, dtype=torch.float64, device=dev) if std is None else std.to(dev).double().reshape(c)
    a = zonal / float(steps * width)
    masks = {name: band_rows(lats_deg, iv) for name, iv in bands.items()}
    for name, m in masks.items():
        if m.numel() != h:
            raise _lib.DlwpError(f"band {name!r}: {m.numel()} latitudes given, the sums have {h} rows")
    d2 = ((a[0] - a[1]) * scale.view(1, c, 1)) ** 2                                   # [B, C, H]
    squares = [(d2 * m.to(dev).view(1, 1, h)).sum(dim=(0, 2)) for m in masks.values()]  # [C] each
    mean = None
    if window is not None and n_window_steps > 0:
        mean = window / float(n_window_steps)
        squares.append((((mean[0] - mean[1]) * scale.view(1, c, 1, 1)) ** 2).sum(dim=(0, 2, 3)))
    buf = torch.cat(squares + [torch.full((1,), float(b), dtype=torch.float64, device=dev)])
    if all_reduce is not None:
        buf = all_reduce(buf)
    n = buf[-1]
    rmse = {name: torch.sqrt(buf[i * c:(i + 1) * c] / (n * float(int(m.sum()))))     # 0 / 0 = NaN for an empty band
            for i, (name, m) in enumerate(masks.items())}
    rmse_window = torch.sqrt(buf[len(masks) * c:(len(masks) + 1) * c] / (n * float(h * width))) if mean is not None else None
    return {"zonal_mean_pred": a[0], "zonal_mean_true": a[1],
            "window_mean_pred": mean[0] if mean is not None else None, "window_mean_true": mean[1] if mean is not None else None,
            "rmse": rmse, "rmse_window": rmse_window}


class SoundnessMetrics(_Scorer):
    """The physical-soundness evaluation of reference scripts/evaluate.py:832-872 for rollouts of any length, streamed: feed the
    rollout and its truth chunk by chunk (`update`), in step order, and `finalize` gives the RMSE of the time-and-longitude mean
    per latitude band (global, trade winds, south westerlies by default) and the RMSE of the field averaged over the lead-time
    window (days 334-365, "months 11-12").  Only the running sums live on the device -- double [2, B, C, H] and, from the
    first chunk that reaches the window, [2, B, C, H, W] -- and dlwp_climate_sums_acc_f32 adds a chunk to them in one launch that
    reads it once, in an order that makes the sums bit-identical however the horizon is cut into chunks.  Nothing is copied to
    the host per chunk.

    `step_days`: the model's time step in days (rollout step k has lead time (k + 1) step_days, evaluate.py:346-347).  `std`:
    the per-variable de-normalisation scale [C] of evaluate.py:281-296, as in RolloutMetrics (the means cancel).  `bands`:
    {name: None or [(lat_lo, lat_hi), ...]}, closed intervals.  With `lons_deg` HEALPix chunks [B, K, C, 12, n, n] are taken too
    and remapped to (lats_deg, lons_deg) on the device (see `_Scorer`); without it they are refused.  Samples are sharded over
    ranks: `finalize(world_size)` moves the squares and the sample count in ONE all-reduce."""

    def __init__(self, lats_deg, step_days: float, std: Optional[torch.Tensor] = None, bands=None, window_days=(334.0, 365.0),
                 group=None, lons_deg=None, max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        super().__init__(lats_deg, lons_deg, max_workspace_bytes, group)
        self.height = len(self._lats)
        self.step_days = float(step_days)
        self.window_days = (float(window_days[0]), float(window_days[1]))
        self.window = window_steps(self.step_days, self.window_days)      # rollout steps [first, last + 1)
        self.bands = dict(DEFAULT_BANDS if bands is None else bands)
        self.std = std.detach().double() if std is not None else None
        self.reset()

    def reset(self):
        self.steps = 0            # rollout steps seen so far
        self.n_window_steps = 0   # of them, in the lead-time window
        self._geom = None         # (B, C, H, W, device) of the first chunk
        self._zonal = None
        self._window = None
        return self

    def chunk_window(self, step_begin: int, steps: int):
        """[win_begin, win_end) of a chunk of `steps` steps whose first is rollout step `step_begin`: its steps in the window"""
        lo = min(max(self.window[0] - step_begin, 0), steps)
        hi = min(max(self.window[1] - step_begin, 0), steps)
        return (lo, hi) if hi > lo else (0, 0)

    def state(self):
        """The accumulators, to checkpoint a long evaluation: {"zonal", "window", "steps", "n_window_steps", "width"}"""
        return {"zonal": self._zonal, "window": self._window, "steps": self.steps, "n_window_steps": self.n_window_steps,
                "width": self._geom[3] if self._geom else None}

    def load_state(self, state):
        """Takes accumulators as `state()` gives them (tensors on any device: `finalize` is plain torch)."""
        z, w = state["zonal"], state["window"]
        if z.dim() != 4 or z.shape[0] != 2 or z.shape[3] != self.height or z.dtype != torch.float64:
            raise _lib.DlwpError(f"zonal sums must be double [2, B, C, {self.height}], got {z.dtype} {tuple(z.shape)}")
        width = int(state["width"])
        if w is not None and (tuple(w.shape) != tuple(z.shape) + (width,) or w.dtype != torch.float64 or w.device != z.device):
            raise _lib.DlwpError(f"window sums must be double {tuple(z.shape) + (width,)} on {z.device}")
        self._zonal, self._window = z, w
        self.steps, self.n_window_steps = int(state["steps"]), int(state["n_window_steps"])
        self._geom = (z.shape[1], z.shape[2], z.shape[3], width, z.device)
        return self

    def update(self, out: torch.Tensor, target: torch.Tensor, step_begin: int):
        """Adds a chunk [B, K, C, H, W] (or HEALPix [B, K, C, 12, n, n], see `lons_deg`) of K consecutive rollout steps, the first
        of which is rollout step `step_begin`.  Chunks arrive in step order, each with the same B, C, H, W on one device."""
        b, k, c, h, w = self._pair_shape(out, target)
        if int(step_begin) != self.steps:
            raise _lib.DlwpError(f"chunks must arrive in order: this one starts at rollout step {step_begin}, "
                                 f"{self.steps} steps have been seen")
        if h != self.height:
            raise _lib.DlwpError(f"{h} latitudes in the chunk, {self.height} given to the metric")
        if self.std is not None and self.std.numel() != c:
            raise _lib.DlwpError(f"{c} variables in the chunk, {self.std.numel()} scales given to the metric")
        if min(b, k, c, h, w) < 1:
            raise _lib.DlwpError(f"empty chunk {tuple(out.shape)}")
        if self._geom is not None and (b, c, h, w) != self._geom[:4]:
            raise _lib.DlwpError(f"chunk with (B, C, H, W) = {(b, c, h, w)} after chunks with {self._geom[:4]}")
        dev = self._pair_device(out, target)
        if self._geom is not None and dev != self._geom[4]:
            raise _lib.DlwpError(f"the chunk is on {dev}, the sums on {self._geom[4]}: one device is needed")
        wb, we = self.chunk_window(self.steps, k)
        if self._geom is None:
            self._geom = (b, c, h, w, dev)
            self._zonal = torch.zeros(2, b, c, h, dtype=torch.float64, device=dev)
        if we > wb and self._window is None:                 # on first need: most chunks of a year never reach the window
            self._window = torch.zeros(2, b, c, h, w, dtype=torch.float64, device=dev)
        win = self._window if we > wb else None
        if out.dim() == 5:
            _lib.launch("dlwp_climate_sums_acc_f32", dev, out.contiguous(), target.contiguous(), self._zonal, win,
                        b, k, c, h, w, wb, we)
        else:
            b0 = 0
            for o, t in self._remapped_chunks(out, target):   # m samples at a time
                m = o.shape[0]
                if m == b:
                    _lib.launch("dlwp_climate_sums_acc_f32", dev, o, t, self._zonal, win, b, k, c, h, w, wb, we)
                else:   # the entry point's sums are [2, m, ...]: the samples' slices go through a contiguous copy, bit for bit
                    z = self._zonal[:, b0:b0 + m].contiguous()
                    ww = win[:, b0:b0 + m].contiguous() if win is not None else None
                    _lib.launch("dlwp_climate_sums_acc_f32", dev, o, t, z, ww, m, k, c, h, w, wb, we)
                    self._zonal[:, b0:b0 + m].copy_(z)
                    if ww is not None:
                        win[:, b0:b0 + m].copy_(ww)
                b0 += m
        self.steps += k
        self.n_window_steps += we - wb
        return self

    def finalize(self, world_size: int = 1):
        """{"zonal_mean_pred", "zonal_mean_true": [B, C, H], "window_mean_pred", "window_mean_true": [B, C, H, W] or None (this
        rank's samples), "rmse": {band: [C]}, "rmse_window": [C] or None (ALL ranks' samples)}, float64 on the sums' device.  A
        rollout that never reached the window gives None for the window's entries.  With world_size > 1 ONE all-reduce moves
        [the sum of squares of every score, the sample count] (shards may differ in size)."""
        if self._zonal is None or self.steps == 0:
            raise _lib.DlwpError("finalize() before any chunk: call update() first")
        return soundness_scores(self._zonal, self._window, self.steps, self.n_window_steps, self._geom[3], self._lats, self.bands,
                                self.std, all_reduce=self._reduce if world_size > 1 else None)


EARTH_RADIUS_M = 1000 * (6357 + 6378) / 2   # reference scripts/losses.py:13
MELR_EPS = 1e-10                            # losses.py:117, absolute


def circumference_weights(lats_deg: torch.Tensor) -> torch.Tensor:
    """cos(lat_h) * 2 pi R in float64: the length of each circle of latitude (losses.py:20-23)."""
    return torch.cos(lats_deg.double() * (math.pi / 180)) * (2 * math.pi * EARTH_RADIUS_M)


class ZonalSpectrumMetrics(_Scorer):
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
        self.circ = circumference_weights(torch.as_tensor(lats_deg))
        self.height = int(self.circ.numel())
        super().__init__(lats_deg, lons_deg, max_workspace_bytes, group, (self.circ,))

    def sums(self, out: torch.Tensor, target: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
        """double [2, K, C, W//2 + 1]: 0 = sum over this rank's samples and latitudes of circ_h P(out), 1 = of P(target)
        (dlwp_zonal_power_sums_f32).  `into`: a [2, K, C, W//2 + 1] double tensor of running sums the new ones are ADDED to
        (dlwp_zonal_power_sums_acc_f32); it is returned.  A HEALPix rollout [B, K, C, 12, n, n] (see `lons_deg`) is remapped chunk
        by chunk and summed into zero-initialised (or `into`) sums."""
        b, k, c, h, w = self._check_pair(out, target)
        nb = w // 2 + 1
        if out.dim() == 6:
            return self._healpix_sums(out, target, into, (2, k, c, nb))
        if h != self.height:
            raise _lib.DlwpError(f"zonal spectrum: {h} latitudes in the rollout, {self.height} given to the metric")
        out, target = out.contiguous(), target.contiguous()
        dev = out.device
        if into is not None:
            _lib.require_running_sums(into, (2, k, c, nb), dev)
        circ, = self._on(dev)
        ws = self._workspace(dev, _lib.load().dlwp_zonal_power_workspace_bytes(b, k, c, h, w))
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
            s, n_samples = self._reduce_sums(s, n_samples)
        energy = s / (n_samples * self.height)
        log_ratio = torch.log((energy[0] + MELR_EPS) / (energy[1] + MELR_EPS))
        return {"energy_pred": energy[0], "energy_true": energy[1], "log_ratio": log_ratio, "melr": log_ratio.mean(dim=-1)}


class SphericalSpectrumMetrics(_Scorer):
    """Power per total wavenumber l of a rollout [B, K, C, nlat, nlon], of its targets and of their difference, and the
    spectral coherence between rollout and target, on `grid` ("legendre-gauss", "equiangular" or "equiangular-centred": the
    cell-centred lat-lon grids of the data, healpix.reference_grid), reduced on the device by one fused transform-and-reduce
    kernel (ops.sph_power_sums, dlwp_sph_power_sums_f32).  The reference has no spherical spectrum: PARITY
    UNPINNED, the definitions are those of sphere.py -- orthonormal harmonics, Condon-Shortley phase, row 0 the northernmost.

    With c = sht(x) and f_m = 1 for m = 0 and 2 m = nlon, else 2:  power(x)[l] = sum_{m <= l} f_m |c[l, m]|^2 and
    cross(x, y)[l] = sum_{m <= l} f_m Re(c_x conj c_y); the sums are [4, K, C, lmax] over the samples: power(out), power(target),
    power(out - target) -- the difference formed in the field domain, where a forecast close to its truth keeps its accuracy --
    and cross(out, target).  With an exact quadrature and a band-limited field the degrees of power(x) add up to the integral
    of x^2 over the sphere, so `finalize` divides by 4 pi n_samples: the degrees of a spectrum add up to the mean square.
    lmax defaults to nlat, mmax to min(lmax, nlon / 2 + 1); on the two equiangular grids the quadrature is exact only for
    l + l' <= nlat - 1, so lmax = nlat / 2 is the largest without aliasing.

    A north-south flip of BOTH inputs on a symmetric grid changes none of the four sums (only the signs of the coefficients
    with odd l - m change): WeatherBench stores south first, and may be scored as stored.

    With `lons_deg` (nlon longitudes) HEALPix rollouts [B, K, C, 12, n, n] are taken too: they are remapped to
    (sphere.latitudes_deg(grid, nlat), lons_deg) on the device in chunks of samples whose lat-lon copies stay within
    `max_workspace_bytes`, and accumulated; without it they are refused.  The target grid is free there: "legendre-gauss" is
    the one to take, its quadrature is exact up to lmax = nlat."""

    def __init__(self, grid: str, nlat: int, nlon: int, lmax: Optional[int] = None, mmax: Optional[int] = None, group=None,
                 lons_deg=None, max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        from . import sphere as _sph

        self.grid, self.nlat, self.nlon = grid, int(nlat), int(nlon)
        self.lmax = self.nlat if lmax is None else int(lmax)
        self.mmax = min(self.lmax, self.nlon // 2 + 1) if mmax is None else int(mmax)
        _sph.check_range(self.nlat, self.nlon, self.lmax, self.mmax)
        super().__init__(_sph.latitudes_deg(grid, self.nlat), lons_deg, max_workspace_bytes, group)
        if self._lons is not None and len(self._lons) != self.nlon:
            raise _lib.DlwpError(f"spherical spectrum: {len(self._lons)} longitudes in lons_deg, nlon = {self.nlon}")

    def sums(self, out: torch.Tensor, target: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
        """double [4, K, C, lmax] sums over this rank's samples (see the class; dlwp_sph_power_sums_f32).  `into`: a
        [4, K, C, lmax] double tensor of running sums the new ones are ADDED to (dlwp_sph_power_sums_acc_f32); it is returned.  A
        HEALPix rollout [B, K, C, 12, n, n] (see `lons_deg`) is remapped chunk by chunk and summed into zero-initialised (or
        `into`) sums: the chain of every sum runs over the samples in order, so the chunk size does not change a bit."""
        from . import ops as _ops

        b, k, c, h, w = self._check_pair(out, target)
        if out.dim() == 6:
            return self._healpix_sums(out, target, into, (4, k, c, self.lmax))
        if (h, w) != (self.nlat, self.nlon):
            raise _lib.DlwpError(f"spherical spectrum: a {h}x{w} rollout, the metric was built for {self.nlat}x{self.nlon}")
        ws = self._workspace(out.device, _ops.sph_power_workspace_bytes(out.shape, self.lmax, self.mmax))
        return _ops.sph_power_sums(out, target, self.grid, self.lmax, self.mmax, into=into, workspace=ws)

    def __call__(self, out: torch.Tensor, target: torch.Tensor, world_size: int = 1):
        """Spectra, coherence and log ratio over ALL ranks' samples (see finalize)."""
        return self.finalize(self.sums(out, target), float(out.shape[0]), world_size)

    def finalize(self, s: torch.Tensor, n_samples: float, world_size: int = 1):
        """Scores from accumulated sums: `s` = this rank's [4, K, C, lmax] sums (of one batch or added up over many),
        n_samples = how many samples went into them.  With world_size > 1 ONE all-reduce moves the sums and the sample count
        (shards may differ in size).  With P = s / (4 pi n) returns, in float64,
          "power_pred", "power_true", "power_error"  [K, C, lmax]   P[0], P[1], P[2]
          "coherence"  [K, C, lmax]   s[3] / sqrt(s[0] s[1]), 0 where the product is 0
          "log_ratio"  [K, C, lmax]   ln((power_pred + 1e-10) / (power_true + 1e-10))   (MELR_EPS)
          "selr"       [K, C]         the mean of log_ratio over l."""
        if world_size > 1:
            s, n_samples = self._reduce_sums(s, n_samples)
        power = s[:3] / (n_samples * (4.0 * math.pi))
        prod = s[0] * s[1]
        coherence = torch.where(prod > 0, s[3] / torch.sqrt(torch.where(prod > 0, prod, torch.ones_like(prod))),
                                torch.zeros_like(prod))
        log_ratio = torch.log((power[0] + MELR_EPS) / (power[1] + MELR_EPS))
        return {"power_pred": power[0], "power_true": power[1], "power_error": power[2], "coherence": coherence,
                "log_ratio": log_ratio, "selr": log_ratio.mean(dim=-1)}


def ensemble_scores(sums: torch.Tensor, ranks: torch.Tensor, count: torch.Tensor, members: int, cells: int):
    """The ensemble scores from accumulated sums (dlwp_ensemble_sums_acc_f32), in plain torch on whatever device they are on:
    sums double [4, K, C], ranks int64 [K, C, M + 1], count double [K] (the samples that went into each step), cells = H W.
    With N = count cells:
      rmse_mean = sqrt(s0 / N)                         RMSE of the ensemble mean
      spread = sqrt(s1 / N)                            root of the mean ensemble variance (1 / (M - 1) form)
      spread_skill = sqrt((M + 1) / M) spread / rmse_mean      1 for a statistically consistent ensemble (Fortin et al. 2014)
      crps = (s2 - s3 / (M (M - 1))) / N               the fair CRPS (Ferro et al. 2008)
      crps_ens = (s2 - s3 / M^2) / N                   the CRPS of the ensemble's own empirical distribution
    all [K, C] double, and rank_histogram = ranks.  A step no sample reached gives NaN."""
    m = int(members)
    n = (count.double() * float(cells)).view(-1, 1)
    rmse_mean = torch.sqrt(sums[0] / n)
    spread = torch.sqrt(sums[1] / n)
    return {"rmse_mean": rmse_mean, "spread": spread, "spread_skill": math.sqrt((m + 1) / m) * spread / rmse_mean,
            "crps": (sums[2] - sums[3] / float(m * (m - 1))) / n, "crps_ens": (sums[2] - sums[3] / float(m * m)) / n,
            "rank_histogram": ranks}


class EnsembleMetrics(_Scorer):
    """Scores of an ensemble forecast [M, B, k, C, H, W] against its truth [B, k, C, H, W], streamed: feed chunks of lead steps
    and / or of samples (`update`), `finalize` gives the latitude-weighted RMSE of the ensemble mean, the spread, their
    ratio, the CRPS (fair and plain) and the rank histogram per lead step and variable.  Only the running sums -- double
    [4, steps, C], int64 [steps, C, M + 1] and the per-step sample count -- live on the device; dlwp_ensemble_sums_acc_f32 adds a
    chunk to them in one call that reads every member value once, sorts the members of a grid point in registers and writes
    nothing of the ensemble's size.  Sums are fp64 in a fixed order: two evaluations give the same bits.  NaNs are not treated.

    PARITY UNPINNED: the reference holds only a commented sketch of an ensemble evaluation (scripts/train.py:352-371: the
    ensemble mean and a standard deviation); the scores here are the usual ensemble-verification forms (see `ensemble_scores`)
    and are pinned by the float64 restatement in the tests, not by the reference.

    `members`: M, 2 to 64.  `steps`, `channels`: the lead steps and variables of the whole evaluation.  `std`: the per-variable
    de-normalisation scale [C] as in RolloutMetrics.  With `lons_deg` HEALPix ensembles [M, B, k, C, 12, n, n] are taken too and
    remapped to (lats_deg, lons_deg) on the device, a chunk of samples -- all members of each -- at a time within
    `max_workspace_bytes`.  Samples are sharded over ranks: `finalize(world_size)` moves sums, ranks and counts in ONE
    all-reduce."""

    def __init__(self, lats_deg, members: int, steps: int, channels: int, std: Optional[torch.Tensor] = None, group=None,
                 lons_deg=None, max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        self.members, self.steps, self.channels = int(members), int(steps), int(channels)
        if not 2 <= self.members <= 64:
            raise _lib.DlwpError(f"EnsembleMetrics: {self.members} members (2 to 64 are supported)", status=_lib.ERR_UNSUPPORTED)
        if self.steps < 1 or self.channels < 1:
            raise _lib.DlwpError(f"EnsembleMetrics: steps = {self.steps} and channels = {self.channels} must be positive")
        self.latw = latitude_weights(torch.as_tensor(lats_deg).reshape(-1))
        self.height = int(self.latw.numel())
        self.std = std.detach().float().reshape(-1) if std is not None else None
        if self.std is not None and self.std.numel() != self.channels:
            raise _lib.DlwpError(f"EnsembleMetrics: {self.std.numel()} scales given for {self.channels} variables")
        super().__init__(lats_deg, lons_deg, max_workspace_bytes, group, (self.latw, self.std))
        self.reset()

    def reset(self):
        self._sums = self._ranks = self._count = None
        self._width = len(self._lons) if self._lons is not None else None
        return self

    def state(self):
        """The accumulators, to checkpoint a long evaluation: {"sums", "ranks", "count", "width"}"""
        return {"sums": self._sums, "ranks": self._ranks, "count": self._count, "width": self._width}

    def _check_state(self, s, r, n):
        k, c, m = self.steps, self.channels, self.members
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float64 or tuple(s.shape) != (4, k, c):
            raise _lib.DlwpError(f"sums must be a double [4, {k}, {c}] tensor, got "
                                 f"{getattr(s, 'dtype', type(s))} {tuple(getattr(s, 'shape', ()))}")
        if not isinstance(r, torch.Tensor) or r.dtype != torch.int64 or tuple(r.shape) != (k, c, m + 1) or r.device != s.device:
            raise _lib.DlwpError(f"ranks must be an int64 [{k}, {c}, {m + 1}] tensor on {s.device}")
        if not isinstance(n, torch.Tensor) or n.dtype != torch.float64 or tuple(n.shape) != (k,) or n.device != s.device:
            raise _lib.DlwpError(f"count must be a double [{k}] tensor on {s.device}")

    def load_state(self, state):
        """Takes accumulators as `state()` gives them (tensors on any device: `finalize` is plain torch)."""
        self._check_state(state["sums"], state["ranks"], state["count"])
        width = int(state["width"])
        if width < 1 or (self._lons is not None and width != len(self._lons)):
            raise _lib.DlwpError(f"width {width} does not fit the metric's grid")
        self._sums, self._ranks, self._count, self._width = state["sums"], state["ranks"], state["count"], width
        return self

    def _launch(self, ens, member_stride, target, b, k, h, w, step_begin):
        dev = target.device
        latw, std = self._on(dev)
        ws = self._workspace(dev, _lib.load().dlwp_ensemble_sums_workspace_bytes(b, k, self.channels, h, w))
        _lib.launch("dlwp_ensemble_sums_acc_f32", dev, ens, target, latw, std, self._sums, self._ranks, self.members, member_stride,
                    b, k, self.channels, h, w, self.steps, step_begin, ws, ws.numel())

    def update(self, ens: torch.Tensor, target: torch.Tensor, step_begin: int = 0):
        """Adds a chunk: ens [M, B, k, C, H, W] (each member contiguous; the members may be any stride apart, e.g. a group view
        of a wider buffer) or HEALPix [M, B, k, C, 12, n, n] (see `lons_deg`) with target [B, k, C, ...], the k consecutive lead
        steps from `step_begin`.  Chunks may arrive in any order; every one counts B samples for its steps."""
        if not isinstance(ens, torch.Tensor) or ens.dim() not in (6, 7) or ens.shape[0] != self.members:
            raise _lib.DlwpError(f"expected an ensemble [{self.members}, B, k, C, H, W], got "
                                 f"{tuple(ens.shape) if isinstance(ens, torch.Tensor) else type(ens)}")
        b, k, c, h, w = self._check_pair(ens[0], target, "ens", "M, ")      # a member and the target are a pair
        m, step_begin = self.members, int(step_begin)
        if h != self.height:
            raise _lib.DlwpError(f"{h} latitudes in the chunk, {self.height} given to the metric")
        if c != self.channels:
            raise _lib.DlwpError(f"{c} variables in the chunk, {self.channels} given to the metric")
        if min(b, k, w) < 1:
            raise _lib.DlwpError(f"empty chunk {tuple(ens.shape)}")
        if step_begin < 0 or step_begin + k > self.steps:
            raise _lib.DlwpError(f"steps [{step_begin}, {step_begin + k}) outside the {self.steps} steps of the metric")
        if self._width is not None and w != self._width:
            raise _lib.DlwpError(f"{w} longitudes in the chunk after chunks with {self._width}")
        dev = ens.device
        if self._sums is None:
            self._sums = torch.zeros(4, self.steps, c, dtype=torch.float64, device=dev)
            self._ranks = torch.zeros(self.steps, c, m + 1, dtype=torch.int64, device=dev)
            self._count = torch.zeros(self.steps, dtype=torch.float64, device=dev)
        elif self._sums.device != dev:
            raise _lib.DlwpError(f"the chunk is on {dev}, the sums on {self._sums.device}: one device is needed")
        self._width = w
        if target.dim() == 5:
            if not ens[0].is_contiguous() or (m > 1 and ens.stride(0) < ens[0].numel()):
                ens = ens.contiguous()
            self._launch(ens, int(ens.stride(0)), target.contiguous(), b, k, h, w, step_begin)
        else:
            for *e, t in self._remapped_chunks(*ens, target):   # all members of a sample in one chunk, a chunk in one call
                stride = e[1].storage_offset() - e[0].storage_offset()      # the members' block: see _remapped_chunks
                self._launch(e[0], stride, t, t.shape[0], k, h, w, step_begin)
        self._count[step_begin:step_begin + k] += float(b)
        return self

    def finalize(self, world_size: int = 1):
        """{"rmse_mean", "spread", "spread_skill", "crps", "crps_ens": [steps, C] double, "rank_histogram": [steps, C, M + 1]
        int64} over ALL ranks' samples (see `ensemble_scores`), on the sums' device.  With world_size > 1 ONE all-reduce moves
        sums, ranks and counts (the rank counts travel as doubles: exact below 2^53)."""
        if self._sums is None:
            raise _lib.DlwpError("finalize() before any chunk: call update() or load_state() first")
        self._check_state(self._sums, self._ranks, self._count)
        s, r, n = self._sums, self._ranks, self._count
        if world_size > 1:
            buf = self._reduce(torch.cat([s.flatten(), r.flatten().double(), n]))
            s = buf[:s.numel()].view_as(s)
            r = buf[s.numel():s.numel() + r.numel()].round().long().view_as(r)
            n = buf[s.numel() + r.numel():]
        return ensemble_scores(s, r, n, self.members, self.height * self._width)
