"""numpy restatement of the reference's WeatherBenchDataset (data/datasets/datasets.py) and of the monthly climatology forecast
(climatology.py:41, scripts/build_baselines.py:35-69), for data held in arrays instead of xarray datasets.  PARITY UNPINNED:
xarray, zarr and netCDF4 are not installed where these tests run; each function cites the lines it restates.

A dataset here is: fields name -> [T, (L,) ...spatial] float32, times datetime64 [T], levels name -> level values.  Where the
reference reduces (mean, std, groupby mean, coarsen) the restatement reduces in float64 (long double for the sums a test
bounds tightly).  The windows are the fixed-length ones of dlwp_benchmark_amd.data (its documented difference from the
reference's label slices): S + 1 consecutive used times."""
import numpy as np


def used_indices(times, start, stop, timedelta):
    """.sel(time=slice(start_date, stop_date, timedelta)) (:291): label-inclusive on both ends, then every timedelta-th"""
    times = np.asarray(times).astype("datetime64[ns]")
    keep = np.nonzero((times >= np.datetime64(start, "ns")) & (times <= np.datetime64(stop, "ns")))[0]
    return keep[::timedelta]


def length(n_used, sequence_length, init_dates=None):
    """:323-328"""
    if init_dates is None:
        return (n_used - sequence_length) // sequence_length
    return len(init_dates)


def window(used, used_times, item, sequence_length, init_dates=None):
    """store indices of the S + 1 frames of one item, -1 past the end: isel(time=slice(item * S, item * S + S + 1)) in index
    mode (:336, :384); from the first used time at or after the init date (the lower bound of the label slice, :387-388)"""
    if init_dates is None:
        start = item * sequence_length
    else:
        later = np.nonzero(used_times >= np.datetime64(init_dates[item], "ns"))[0]
        start = int(later[0]) if later.size else len(used)
    out = []
    for j in range(sequence_length + 1):
        out.append(int(used[start + j]) if start + j < len(used) else -1)
    return out


def _select(fields, levels, name, level):
    a = fields[name]
    return a[:, list(levels[name]).index(level)] if level is not None else a


def getitem(fields, levels, frames, prognostic, prescribed, stats, normalize, context_size, constants=None):
    """__getitem__ (:330-416) at noise = 0 for one window given by its S + 1 store indices.  Returns (constants or None,
    prescribed or None, prognostic, target); None is the NaN sentinel (:317, :378)."""
    s = len(frames) - 1
    pres = None
    if prescribed:
        cols = []
        for p in prescribed:
            x = fields[p][frames[:s]]                                                        # :345
            if normalize:
                x = (x - stats[p]["mean"]) / stats[p]["std"]                                 # :371
            cols.append(x)
        pres = np.float32(np.stack(cols, axis=1))                                            # :375
    cols = []
    for p, lv in prognostic.items():
        if p in levels:
            for l in lv:                                                                     # :393-398
                x = _frames_or_zero(_select(fields, levels, p, l), frames)
                if normalize:
                    x = (x - stats[p]["level"][l]["mean"]) / stats[p]["level"][l]["std"]
                    x = np.where(np.isnan(x), np.float32(0), x)
                cols.append(x)
        else:                                                                                # :399-402
            x = _frames_or_zero(fields[p], frames)
            if normalize:
                x = (x - stats[p]["mean"]) / stats[p]["std"]
            x = np.where(np.isnan(x), np.float32(0), x)
            cols.append(x)
    prog = np.float32(np.stack(cols, axis=1))                                                # :403
    for j, f in enumerate(frames):                                                           # :405-409: missing frames are zeros
        if f < 0:
            prog[j] = 0
    target = prog[1:]                                                                        # :413
    return constants, pres, prog[:-1], target[context_size:]                                 # :414 (noise 0), :416


def _frames_or_zero(a, frames):
    """a[frames] with a zero frame for -1 (filled before normalisation here, overwritten with zeros after it by the caller)"""
    out = np.zeros((len(frames),) + a.shape[1:], dtype=np.float32)
    for j, f in enumerate(frames):
        if f >= 0:
            out[j] = a[f]
    assert out.dtype == np.float32
    return out


def collate(samples):
    """default_collate of the four-tuples: stack along a new batch axis, None stays None"""
    return tuple(None if parts[0] is None else np.stack(parts) for parts in zip(*samples))


def constants_block(constants, names, stats, normalize):
    """:308-315: [1, #constants, ...]"""
    out = []
    for c in names:
        x = np.asarray(constants[c], dtype=np.float32)
        if normalize:
            x = (x - stats[c]["mean"]) / stats[c]["std"]
        out.append(x)
    return np.expand_dims(np.float32(np.stack(out)), axis=0)


def statistics(x):
    """(count, sum, squared deviations) of the non-NaN values of a float32 array in float64: xarray's .mean() / .std() skip
    NaN and .std() has ddof 0 (:429, :435, :444, :448).  The sums are long double, so their own error is negligible."""
    v = x[~np.isnan(x)].astype(np.longdouble)
    n = v.size
    s = v.sum()
    mean = np.float64(s / n) if n else np.float64("nan")
    ssd = ((v.astype(np.float64) - mean).astype(np.longdouble) ** 2).sum() if n else np.longdouble(0)
    return n, np.float64(s), np.float64(ssd)


def group_mean(x, groups, n_groups):
    """groupby(...).mean() over axis 0 (climatology.py:41), NaN skipped, in long double; also the sum of |x| per element"""
    out = np.full((n_groups,) + x.shape[1:], np.nan, dtype=np.float64)
    mag = np.zeros((n_groups,) + x.shape[1:], dtype=np.float64)
    for g in range(n_groups):
        sel = x[np.asarray(groups) == g].astype(np.longdouble)
        if sel.shape[0] == 0:
            continue
        ok = ~np.isnan(sel)
        cnt = ok.sum(axis=0)
        tot = np.where(ok, sel, 0).sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[g] = np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan).astype(np.float64)
        mag[g] = np.where(ok, np.abs(sel), 0).sum(axis=0).astype(np.float64)
    return out, mag


def coarsen(x, k):
    """ds.coarsen(lat=k, lon=k).mean() (:303-305), NaN skipped, float64"""
    *lead, h, w = x.shape
    b = x.astype(np.float64).reshape(*lead, h // k, k, w // k, k)
    ok = ~np.isnan(b)
    cnt = ok.sum(axis=(-3, -1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, np.where(ok, b, 0).sum(axis=(-3, -1)) / np.maximum(cnt, 1), np.nan)


def lead_months(init_times, dt, steps):
    """month - 1 of init + (k + 1) dt (scripts/build_baselines.py:65-69 over the coordinates of evaluate.py:346-352)"""
    out = np.zeros((len(init_times), steps), dtype=np.int64)
    for i, t0 in enumerate(init_times):
        for k in range(steps):
            t = np.datetime64(t0, "ns") + (k + 1) * dt
            out[i, k] = int(str(t.astype("datetime64[M]"))[5:7]) - 1
    return out
