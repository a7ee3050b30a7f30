"""The device-resident WeatherBench dataset: the fields are handed over once, batches, evaluation windows, statistics and the
climatology / persistence baselines are drawn from the card (csrc/dataset.hip).

Reference: `WeatherBenchDataset` (data/datasets/datasets.py:16-453), the monthly climatology (climatology.py:41) and
scripts/build_baselines.py:23-72.  PARITY UNPINNED: the reference class needs xarray and zarr / netCDF4 files, none of which
exist where this package is tested; the module is pinned by a numpy restatement of the cited lines (tests/dataset_ref.py).

Replaces `DataLoader(WeatherBenchDataset(...))` + `staging.DeviceStager`: `DeviceWeatherDataset.batches()` yields the tuples
the stager yields -- (constants, prescribed, prognostic, target) device tensors, None where the reference returns its NaN
sentinel -- without a host loader, a collate or an upload.

Deliberate differences from the reference (DESIGN.md section 34 has the reasons):
  * windows have fixed lengths: S + 1 consecutive used times from the first one at or after the init date; the reference's
    label-inclusive `sel` slices mix hour and day units (:350, :389) and its tail pad goes to S, not S + 1 (:405).  A missing
    prognostic frame is zeros.
  * a prescribed frame past the end of the store raises; the copy of a 2022 frame (:354-369) is not restated
    (`rollout.insolation_forcing` generates that variable for any date).
  * the input noise comes from the Philox member stream (seed, member = item, offset = draw * ceil4(S C plane)), not from numpy's
    global generator (:414).  At noise = 0 nothing differs.
  * `compute_statistics()` returns the dict shape the constructor READS (`stats[p]["level"][l]`, :396); the reference's own
    method writes `statistics[p][float(l)]` into a missing key (:446) and cannot return for a variable with levels.
"""
from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from . import ops as _ops


def _ceil4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def _as_time(t, end_of_period: bool = False) -> np.datetime64:
    """a date as datetime64[ns]; with `end_of_period` a value of day (or coarser) resolution -- "2014-12-31" -- names the END of
    that period, as in xarray's label slices (datasets.py:291)"""
    if hasattr(t, "to_datetime64"):      # a pandas Timestamp (tz-aware ones carry UTC instants)
        t = t.tz_convert(None).to_datetime64() if getattr(t, "tzinfo", None) is not None else t.to_datetime64()
    t = np.datetime64(t)
    unit = np.datetime_data(t.dtype)[0]
    if end_of_period and unit in ("Y", "M", "W", "D"):
        return (t + 1).astype("datetime64[ns]") - np.timedelta64(1, "ns")
    return t.astype("datetime64[ns]")


def channel_layout(prognostic_variable_names_and_levels: Dict, prescribed_variable_names: Sequence[str], levels: Dict,
                   normalize: bool):
    """The channels of a batch in the reference's order (datasets.py:339-341, :382-402):
    (prognostic [(name, level or None, nan_fill)], prescribed [(name, None, False)]).  NaN is replaced by 0 always for a
    variable without levels (:401) and only under `normalize` for one with levels (:395-397); never for a prescribed one (:371)."""
    prog = []
    for name, lv in prognostic_variable_names_and_levels.items():
        if name in levels:
            for l in lv:
                if l not in list(levels[name]):
                    raise ValueError(f"{name} has no level {l} (levels: {list(levels[name])})")
                prog.append((name, l, bool(normalize)))
        else:
            prog.append((name, None, True))
    pres = [(name, None, False) for name in prescribed_variable_names]
    return prog, pres


class WindowIndex:
    """The host half of the dataset, pure numpy: which stored times are used and which of them make up a window.
      used        store indices of .sel(time=slice(start_date, stop_date, timedelta)) (datasets.py:291)
      __len__     datasets.py:323-328
      frame_table the S + 1 frames of every item (:336, :345 / :348-349, :384 / :387-389), fixed-length"""

    def __init__(self, times, start_date, stop_date, timedelta: int, init_dates, sequence_length: int):
        self.times = np.asarray(times).astype("datetime64[ns]")
        if self.times.ndim != 1 or self.times.size == 0 or np.any(np.diff(self.times) <= np.timedelta64(0, "ns")):
            raise ValueError("times must be a non-empty ascending datetime64 vector")
        self.timedelta, self.sequence_length = int(timedelta), int(sequence_length)
        if self.timedelta < 1 or self.sequence_length < 1:
            raise ValueError("timedelta and sequence_length must be >= 1")
        lo = int(np.searchsorted(self.times, _as_time(start_date), "left"))
        hi = int(np.searchsorted(self.times, _as_time(stop_date, end_of_period=True), "right"))
        self.used = np.arange(lo, hi, self.timedelta, dtype=np.int64)
        self.used_times = self.times[self.used]
        self.init_dates = None if init_dates is None else np.array([_as_time(t) for t in init_dates], dtype="datetime64[ns]")

    def __len__(self) -> int:
        if self.init_dates is None:
            return max((self.used.size - self.sequence_length) // self.sequence_length, 0)
        return len(self.init_dates)

    def starts(self, items) -> np.ndarray:
        """position of frame 0 of every item on the used time axis"""
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        if items.size and (items.min() < 0 or (self.init_dates is not None and items.max() >= len(self.init_dates))):
            raise IndexError(f"items {items.tolist()} outside the dataset")
        if self.init_dates is None:
            return items * self.sequence_length
        return np.searchsorted(self.used_times, self.init_dates[items], "left").astype(np.int64)

    def frames(self, items, first: int, count: int) -> np.ndarray:
        """int32 [len(items), count]: the store index of the used times first .. first + count - 1 after each window's start,
        -1 past the end"""
        pos = self.starts(items)[:, None] + (int(first) + np.arange(int(count), dtype=np.int64))[None, :]
        ok = (pos >= 0) & (pos < self.used.size)
        out = np.full(pos.shape, -1, dtype=np.int32)
        out[ok] = self.used[pos[ok]]
        return out

    def frame_table(self, items) -> np.ndarray:
        """int32 [len(items), S + 1]: the store time index of every frame of every window, -1 past the end of the used times.
        Index mode: the window starts at item * S on the used (strided) axis; init_dates mode: at the first used time at or
        after the date."""
        return self.frames(items, 0, self.sequence_length + 1)


class BatchBuffers:
    """The fixed addresses of a batch: the device frame table int32 [B, S + 1], the item table int32 [B] and the three outputs
    (any of them may be a caller's contiguous tensor, e.g. a view into a larger arena).  `set_items` overwrites the tables in
    place; `DeviceWeatherDataset.gather` is one launch that reads them when it executes, so a recorded gather follows them."""

    def __init__(self, dataset: "DeviceWeatherDataset", batch_size: int, prescribed=None, prognostic=None, target=None):
        d, b = dataset, int(batch_size)
        if b < 1:
            raise ValueError("batch_size must be >= 1")
        self.dataset, self.batch_size = d, b
        self.frames = torch.full((b, d.sequence_length + 1), -1, dtype=torch.int32, device=d.device)
        self.items = torch.zeros((b,), dtype=torch.int32, device=d.device)

        def flat(t, n, frames):
            shape = (b, frames, n, d.plane)
            if t is None:
                return torch.empty(shape, dtype=torch.float32, device=d.device) if n and frames else None
            _lib.require_cuda_tensor(t, "buffer")
            if not t.is_contiguous() or t.numel() != b * frames * n * d.plane:
                raise _lib.DlwpError(f"a batch buffer must be contiguous with {shape} elements (got {tuple(t.shape)})")
            return t.view(shape)

        s = d.sequence_length
        self.prescribed = flat(prescribed, d.n_prescribed, s)
        self.prognostic = flat(prognostic, d.n_prognostic, s)
        self.target = flat(target, d.n_prognostic, s - d.context_size)

    def set_items(self, items):
        d = self.dataset
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        if items.size != self.batch_size:
            raise ValueError(f"{items.size} items for buffers of batch size {self.batch_size}")
        table = d.frame_table(items)
        d._check_prescribed(table)
        self.frames.copy_(torch.from_numpy(table))
        self.items.copy_(torch.from_numpy(items.astype(np.int32)))


class DeviceWeatherDataset:
    """See the module docstring.  Constructor arguments of the reference (datasets.py:21-41) keep their names and meanings:
    prognostic_variable_names_and_levels, prescribed_variable_names, constant_names, start_date, stop_date, timedelta (the
    stride of the stored time axis, :291), init_dates, sequence_length, noise, normalize, downscale_factor, context_size.

    What replaces the files:
      fields     name -> array [T, (L,) H, W] (lat-lon) or [T, (L,) 12, n, n] (HEALPix); a name listed in `levels` has the L axis
      times      datetime64 [T], ascending: the stored time axis
      levels     name -> the level values along L
      constants  name -> array [H, W] or [12, n, n]
      stats      the reference's table: name -> {"mean", "std"} or {"level": {l: {"mean", "std"}}}; None: computed from the
                 used times by compute_statistics() where `normalize` needs it (none of the reference's tables ships here)
      seed       of the noise stream
    or, for fields that are on the card already, `store` [T, V, plane] float32 with `store_variables` [(name, level or None)]
    and `spatial_shape` in place of `fields` (the store is used as it is: no copy, no coarsening)."""

    def __init__(self, prognostic_variable_names_and_levels: Dict, prescribed_variable_names: Sequence[str] = (),
                 constant_names: Optional[Sequence[str]] = None, start_date=np.datetime64("1979-01-01"),
                 stop_date=np.datetime64("2014-12-31"), timedelta: int = 6, init_dates=None, sequence_length: int = 15,
                 noise: float = 0.0, normalize: bool = False, downscale_factor: int = 1, context_size: int = 2, *,
                 fields: Optional[Dict] = None, times=None, levels: Optional[Dict] = None, constants: Optional[Dict] = None,
                 stats: Optional[Dict] = None, device="cuda", seed: int = 0, store: Optional[torch.Tensor] = None,
                 store_variables: Optional[Sequence] = None, spatial_shape: Optional[Sequence[int]] = None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DlwpError(f"DeviceWeatherDataset keeps its store on a GPU (got {device}); the HIP path has no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.prognostic_variable_names_and_levels = dict(prognostic_variable_names_and_levels)
        self.prescribed_variable_names = list(prescribed_variable_names or [])
        self.constant_names = list(constant_names or [])
        self.timedelta, self.sequence_length, self.context_size = int(timedelta), int(sequence_length), int(context_size)
        self.noise, self.normalize, self.downscale_factor = float(noise), bool(normalize), int(downscale_factor)
        self.seed = int(seed)
        self.levels = {k: list(v) for k, v in (levels or {}).items()}
        if not 0 <= self.context_size <= self.sequence_length:
            raise ValueError("0 <= context_size <= sequence_length is needed")
        if self.downscale_factor < 1:
            raise ValueError("downscale_factor must be >= 1")
        if times is None:
            raise ValueError("times (datetime64 [T]) is needed")
        self.index = WindowIndex(times, start_date, stop_date, self.timedelta, init_dates, self.sequence_length)
        self.times, self.used, self.used_times, self.init_dates = (self.index.times, self.index.used, self.index.used_times,
                                                                   self.index.init_dates)
        self.prog_channels, self.pres_channels = channel_layout(self.prognostic_variable_names_and_levels,
                                                                self.prescribed_variable_names, self.levels, self.normalize)
        self.n_prognostic, self.n_prescribed = len(self.prog_channels), len(self.pres_channels)

        if store is not None:
            self._adopt_store(store, store_variables, spatial_shape)
        else:
            self._build_store(fields or {})
        self._used_dev = torch.from_numpy(self.used.astype(np.int32)).to(self.device)
        self.stats = stats
        if self.normalize and self.stats is None:
            self.stats = self.compute_statistics(constants=constants)
        self._prog_table = self._table(self.prog_channels)
        self._pres_table = self._table(self.pres_channels)
        self.constants = self._prepare_constants(constants)
        self.epoch = 0
        self._climatology = {}

    # ---- construction ---------------------------------------------------------------------------------------------------------
    def _adopt_store(self, store, store_variables, spatial_shape):
        _lib.require_cuda_tensor(store, "store")
        if store.dim() != 3 or not store.is_contiguous() or store.shape[0] != self.times.size or store_variables is None \
                or len(store_variables) != store.shape[1] or spatial_shape is None \
                or int(np.prod(spatial_shape)) != store.shape[2]:
            raise _lib.DlwpError("store must be contiguous [len(times), len(store_variables), prod(spatial_shape)]")
        if self.downscale_factor != 1:
            raise _lib.DlwpError("a store that is handed over is used as it is: coarsen the fields before (ops.coarsen_mean)")
        self.device = store.device
        self.store = store
        self.store_variables = [(n, l) for n, l in store_variables]
        self.spatial_shape = tuple(int(s) for s in spatial_shape)
        self.plane = int(store.shape[2])

    def _build_store(self, fields):
        wanted = []
        for name, lv, _ in self.prog_channels + self.pres_channels:
            if (name, lv) not in wanted:
                wanted.append((name, lv))
        if not wanted:
            raise ValueError("no prognostic or prescribed variable is named")
        k = self.downscale_factor
        planes, spatial = [], None
        for name, lv in wanted:
            if name not in fields:
                raise KeyError(f"fields has no variable {name!r}")
            a = fields[name]
            a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
            if name in self.levels:
                a = a[:, list(self.levels[name]).index(lv)]
            if a.shape[0] != self.times.size or a.dim() not in (3, 4):
                raise ValueError(f"{name}: expected [T = {self.times.size}, (L,) H, W] or [T, (L,) 12, n, n], got {tuple(a.shape)}")
            a = a.to(self.device, dtype=torch.float32)
            if k > 1:
                # datasets.py:303-305: `assert "face" not in self.ds.coords`
                if a.dim() == 4:
                    raise _lib.DlwpError("Downscaling only supported with LatLon and not with HEALPix data.")
                a = _ops.coarsen_mean(a, k)
            if spatial is None:
                spatial = tuple(a.shape[1:])
            elif tuple(a.shape[1:]) != spatial:
                raise ValueError(f"{name}: grid {tuple(a.shape[1:])} differs from {spatial}")
            planes.append(a)
        self.spatial_shape = spatial
        self.plane = int(np.prod(spatial))
        self.store = torch.empty((self.times.size, len(wanted), self.plane), dtype=torch.float32, device=self.device)
        for v, a in enumerate(planes):
            self.store[:, v] = a.reshape(self.times.size, self.plane)
        self.store_variables = wanted

    def _stat(self, name, lv):
        try:
            e = self.stats[name]
            e = e["level"][lv] if lv is not None else e
            return float(e["mean"]), float(e["std"])
        except (KeyError, TypeError) as exc:
            raise KeyError(f"stats has no mean / std for {name!r}" + (f" level {lv}" if lv is not None else "")) from exc

    def _table(self, channels):
        """int32 [n, 4] = {store variable, mean bits, std bits, NaN-fill flag}: the channel table of dlwp_dataset_gather_f32"""
        if not channels:
            return None
        return torch.from_numpy(self.channel_table(channels)).to(self.device)

    def channel_table(self, channels) -> np.ndarray:
        rows = np.zeros((len(channels), 4), dtype=np.int32)
        for i, (name, lv, fill) in enumerate(channels):
            mean, std = self._stat(name, lv) if self.normalize else (0.0, 1.0)
            rows[i, 0] = self.store_variables.index((name, lv))
            rows[i, 1:3] = np.array([mean, std], dtype=np.float32).view(np.int32)
            rows[i, 3] = int(fill)
        return rows

    def _prepare_constants(self, constants):
        """datasets.py:308-317: normalised once, [1, #constants, ...]; None stands for the NaN sentinel"""
        if not self.constant_names:
            return None
        out = []
        for name in self.constant_names:
            if constants is None or name not in constants:
                raise KeyError(f"constants has no field {name!r}")
            c = np.asarray(constants[name], dtype=np.float32)
            if self.downscale_factor > 1:
                c = _ops.coarsen_mean(torch.from_numpy(np.ascontiguousarray(c)).to(self.device), self.downscale_factor).cpu().numpy()
            if tuple(c.shape) != tuple(self.spatial_shape):
                raise ValueError(f"constant {name}: grid {tuple(c.shape)} differs from {tuple(self.spatial_shape)}")
            if self.normalize:
                mean, std = self._stat(name, None)
                c = (c - np.float32(mean)) / np.float32(std)
            out.append(c)
        return torch.from_numpy(np.float32(np.stack(out))[None]).to(self.device)

    # ---- windows --------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        """datasets.py:323-328"""
        return len(self.index)

    def frame_table(self, items) -> np.ndarray:
        """WindowIndex.frame_table: int32 [len(items), S + 1] store time indices, -1 past the end.  Pure numpy."""
        return self.index.frame_table(items)

    def _check_prescribed(self, table):
        if self.n_prescribed and np.any(table[:, :self.sequence_length] < 0):
            raise _lib.DlwpError("a prescribed frame lies past the end of the stored times (the reference copies a 2022 frame, "
                                 "datasets.py:354-369; generate the forcing with rollout.insolation_forcing instead)")

    # ---- batches --------------------------------------------------------------------------------------------------------------
    def buffers(self, batch_size: int, prescribed=None, prognostic=None, target=None) -> BatchBuffers:
        return BatchBuffers(self, batch_size, prescribed, prognostic, target)

    def noise_offset(self, draw: int) -> int:
        return int(draw) * _ceil4(self.sequence_length * self.n_prognostic * self.plane)

    def _shaped(self, t, b):
        return None if t is None else t.view((b, t.shape[1], t.shape[2]) + tuple(self.spatial_shape))

    def gather(self, bufs: BatchBuffers, draw: int = 0):
        """ONE launch from the tables of `bufs` into its outputs; no host value but `draw` goes into it (a recorded gather keeps
        the draw it was recorded with).  Returns (constants, prescribed, prognostic, target)."""
        b = bufs.batch_size
        pres, prog, tar = _ops.dataset_gather(self.store, bufs.frames, self._prog_table, self._pres_table, self.context_size,
                                              self.normalize, self.noise, bufs.items, self.seed, self.noise_offset(draw),
                                              bufs.prescribed, bufs.prognostic, bufs.target)
        const = None if self.constants is None else self.constants.unsqueeze(0).expand((b,) + tuple(self.constants.shape))
        return const, self._shaped(pres, b), self._shaped(prog, b), self._shaped(tar, b)

    def batch(self, items, out: Optional[BatchBuffers] = None, draw: int = 0):
        """default_collate over __getitem__ (datasets.py:330-416) for the dataset items `items`, on the device:
        (constants [B, 1, Cc, ...], prescribed [B, S, P, ...], prognostic [B, S, C, ...], target [B, S - context, C, ...]),
        None where the reference returns its NaN sentinel.  `out`: buffers() to write into (fixed addresses)."""
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        bufs = out if out is not None else BatchBuffers(self, items.size)
        bufs.set_items(items)
        return self.gather(bufs, draw)

    def batches(self, batch_size: int, shuffle: bool = False, generator: Optional[torch.Generator] = None,
                split_size: Optional[int] = None) -> Iterator:
        """One epoch in the order of DataLoader(batch_size, shuffle, generator): torch.randperm(len, generator) on the host when
        shuffling, the last short batch kept; with `split_size` every batch is handed on as consecutive sub-batches (views of
        one gather), as DeviceStager does.  The noise draw advances per epoch."""
        n, draw = len(self), self.epoch
        self.epoch += 1
        order = torch.randperm(n, generator=generator).numpy() if shuffle else np.arange(n)
        for a in range(0, n, int(batch_size)):
            cur = self.batch(order[a:a + int(batch_size)], draw=draw)
            if not split_size:
                yield cur
            else:
                m = max(t.shape[0] for t in cur if t is not None)
                for i in range(0, m, int(split_size)):
                    yield tuple(t[i:i + int(split_size)] if t is not None else None for t in cur)

    def target_chunk(self, items, step_begin: int, steps: int) -> torch.Tensor:
        """[B, steps, C, ...]: the truth of lead steps [step_begin, step_begin + steps) -- bitwise target[:, step_begin :
        step_begin + steps] of a window long enough to hold them -- by the gather kernel (frames past the used times are zeros).
        For rollout.rollout_chunks + SoundnessMetrics / EnsembleMetrics.update: a long evaluation never holds its whole truth."""
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        steps = int(steps)
        if steps < 1 or int(step_begin) < 0:
            raise ValueError("step_begin >= 0 and steps >= 1 are needed")
        table = np.full((items.size, steps + 1), -1, dtype=np.int32)      # column 0: the frame no output asks for
        table[:, 1:] = self.index.frames(items, 1 + self.context_size + int(step_begin), steps)
        frames = torch.from_numpy(table).to(self.device)
        _, _, tar = _ops.dataset_gather(self.store, frames, self._prog_table, None, 0, self.normalize, want_prognostic=False)
        return self._shaped(tar, items.size)

    # ---- statistics and baselines -----------------------------------------------------------------------------------------------
    def compute_statistics(self, constants: Optional[Dict] = None) -> Dict:
        """compute_statistics (datasets.py:419-453) over the used times, NaN skipped, std with ddof 0: two passes of
        dlwp_dataset_stats_f64 over the resident store; mean and std are formed here from (count, sum, squared deviations)."""
        sums = _ops.dataset_stats(self.store, self._used_dev).cpu().numpy()

        def entry(name, row):
            n, s, ssd = row
            return {"file_name": f"{name}", "mean": float(s / n) if n else float("nan"),
                    "std": float(np.sqrt(ssd / n)) if n else float("nan")}

        out = {}
        for name in self.constant_names:
            if constants is None or name not in constants:
                raise KeyError(f"constants has no field {name!r}")
            c = torch.from_numpy(np.ascontiguousarray(constants[name], dtype=np.float32)).to(self.device)
            if self.downscale_factor > 1:
                c = _ops.coarsen_mean(c, self.downscale_factor)
            row = _ops.dataset_stats(c.reshape(1, 1, -1), torch.zeros(1, dtype=torch.int32, device=self.device)).cpu().numpy()[0]
            out[name] = entry(name, row)
        for v, (name, lv) in enumerate(self.store_variables):
            if lv is None:
                out[name] = entry(name, sums[v])
            else:
                out.setdefault(name, {"file_name": f"{name}", "level": {}})["level"][lv] = entry(name, sums[v])
        return out

    def monthly_climatology(self, start="1981-01-01", stop="2010-12-31") -> torch.Tensor:
        """[12, C, ...]: groupby(time.dt.month).mean() of every prognostic channel over the STORED times in [start, stop]
        (climatology.py:16-17, :41; scripts/build_baselines.py:41-42, :64), in the store's units; NaN for a month without data."""
        key = (str(start), str(stop))
        if key not in self._climatology:
            lo = int(np.searchsorted(self.times, _as_time(start), "left"))
            hi = int(np.searchsorted(self.times, _as_time(stop, end_of_period=True), "right"))
            if hi <= lo:
                raise ValueError(f"no stored time in [{start}, {stop}]")
            frames = np.arange(lo, hi, dtype=np.int32)
            months = (self.times[lo:hi].astype("datetime64[M]").astype(np.int64) % 12).astype(np.int32)
            clim = _ops.dataset_group_mean(self.store, torch.from_numpy(frames).to(self.device),
                                           torch.from_numpy(months).to(self.device), 12)
            src = torch.tensor([self.store_variables.index((n, l)) for n, l, _ in self.prog_channels], device=self.device)
            self._climatology[key] = clim.index_select(1, src).contiguous()
        return self._climatology[key].view((12, self.n_prognostic) + tuple(self.spatial_shape))

    def lead_months(self, items, steps: int) -> np.ndarray:
        """int32 [len(items), steps]: month - 1 of init time + (k + 1) dt for k < steps (scripts/build_baselines.py:65-69 with the
        coordinates of evaluate.py:346-352); the init time is the init date, or the time of frame 0 in index mode, and dt the
        spacing of the used times."""
        items = np.asarray(items, dtype=np.int64).reshape(-1)
        if self.init_dates is not None:
            t0 = self.init_dates[items]
        else:
            t0 = self.used_times[np.clip(self.index.starts(items), 0, self.used.size - 1)]
        dt = self.used_times[1] - self.used_times[0] if self.used.size > 1 else np.timedelta64(0, "ns")
        valid = t0[:, None] + dt * (1 + np.arange(int(steps), dtype=np.int64))[None, :]
        return (valid.astype("datetime64[M]").astype(np.int64) % 12).astype(np.int32)

    def climatology_forecast(self, items, steps: int, start="1981-01-01", stop="2010-12-31") -> torch.Tensor:
        """[B, steps, C, ...]: the climatology of the month each lead step falls into (scripts/build_baselines.py:35-69): the
        gather kernel over the 12-frame climatology, copying (no normalisation, no fill)."""
        clim = self.monthly_climatology(start, stop).reshape(12, self.n_prognostic, self.plane)
        months = self.lead_months(items, steps)
        table = np.full((months.shape[0], int(steps) + 1), -1, dtype=np.int32)
        table[:, 1:] = months
        ident = np.zeros((self.n_prognostic, 4), dtype=np.int32)
        ident[:, 0] = np.arange(self.n_prognostic)
        _, _, out = _ops.dataset_gather(clim, torch.from_numpy(table).to(self.device), torch.from_numpy(ident).to(self.device),
                                        None, 0, False, want_prognostic=False)
        return self._shaped(out, months.shape[0])

    def persistence_forecast(self, prognostic: torch.Tensor, steps: int) -> torch.Tensor:
        """[B, steps, C, ...]: the last context frame at every lead step (scripts/build_baselines.py:23-28).  A broadcast view."""
        last = prognostic[:, self.context_size - 1 if self.context_size else 0]
        return last.unsqueeze(1).expand((last.shape[0], int(steps)) + tuple(last.shape[1:]))

    @classmethod
    def from_xarray(cls, ds, prognostic_variable_names_and_levels, prescribed_variable_names=(), constant_names=None, **kwargs):
        """Convenience for a machine that has xarray: `ds` as xr.open_mfdataset(...) returns it (datasets.py:291, unsliced).  Reads
        every named variable into host memory once and hands the arrays over.  UNTESTED: xarray is not installed where this
        package's tests run; nothing else in the package depends on this method."""
        try:
            import xarray  # noqa: F401
        except ImportError as e:
            raise ImportError("DeviceWeatherDataset.from_xarray needs xarray; pass fields= / times= arrays instead") from e
        names = list(prognostic_variable_names_and_levels) + list(prescribed_variable_names or [])
        fields = {n: np.asarray(ds[n].values, dtype=np.float32) for n in names}
        levels = {n: [l for l in ds[n].level.values.tolist()] for n in names if "level" in ds[n].coords and ds[n].level.ndim}
        constants = {n: np.asarray(ds[n].values, dtype=np.float32) for n in (constant_names or [])}
        return cls(prognostic_variable_names_and_levels, prescribed_variable_names, constant_names, fields=fields,
                   times=ds.time.values, levels=levels, constants=constants, **kwargs)
