"""Host half of the device-resident dataset (dlwp_benchmark_amd/data.py): window indexing, length, channel layout and NaN-fill
flags against the numpy restatement of the reference (tests/dataset_ref.py).  No GPU."""
import numpy as np
import pytest

import dataset_ref as R
from dlwp_benchmark_amd.data import WindowIndex, channel_layout

TIMES = np.arange("2000-01-01", "2000-03-01", np.timedelta64(6, "h"), dtype="datetime64[h]")      # 240 stored times


def _ref_table(times, start, stop, td, s, init_dates, items):
    used = R.used_indices(times, start, stop, td)
    used_times = np.asarray(times).astype("datetime64[ns]")[used]
    return np.array([R.window(used, used_times, i, s, init_dates) for i in items], dtype=np.int32)


@pytest.mark.parametrize("td", [1, 3])
@pytest.mark.parametrize("s", [1, 4])
def test_frame_table_index_mode(td, s):
    start, stop = np.datetime64("2000-01-03T06"), np.datetime64("2000-02-20T18")
    w = WindowIndex(TIMES, start, stop, td, None, s)
    used = R.used_indices(TIMES, start, stop, td)
    assert np.array_equal(w.used, used)
    n = len(w)
    assert n == R.length(len(used), s) and n > 2
    items = [0, 1, n // 2, n - 1]                                   # the last valid item included
    got = w.frame_table(items)
    assert got.dtype == np.int32 and got.shape == (4, s + 1)
    assert np.array_equal(got, _ref_table(TIMES, start, stop, td, s, None, items))
    assert (got >= 0).all()                                         # every valid item has all of its S + 1 frames
    assert np.array_equal(np.diff(got, axis=1), np.full((4, s), td))


def test_frame_table_runs_past_the_end():
    start, stop = np.datetime64("2000-01-01"), np.datetime64("2000-01-10T18")      # 40 used times at td = 1
    w = WindowIndex(TIMES, start, stop, 1, None, 7)
    assert len(w) == (40 - 7) // 7 == 4
    got = w.frame_table([5])                                        # frames 35 .. 42: five exist
    assert np.array_equal(got, _ref_table(TIMES, start, stop, 1, 7, None, [5]))
    assert got[0].tolist() == [35, 36, 37, 38, 39, -1, -1, -1]
    assert (w.frame_table([6]) == -1).all()


def test_a_date_only_stop_covers_its_whole_day():
    """xarray's label slice with "2000-01-10" runs to the end of that day (datasets.py:291)"""
    w = WindowIndex(TIMES, "2000-01-01", "2000-01-10", 1, None, 3)
    assert w.used.size == 40 and w.used[-1] == 39
    w = WindowIndex(TIMES, np.datetime64("2000-01-01"), np.datetime64("2000-01-10T00"), 1, None, 3)
    assert w.used.size == 37


@pytest.mark.parametrize("td", [1, 3])
def test_frame_table_init_dates_between_stored_times(td):
    start, stop = np.datetime64("2000-01-02T00"), np.datetime64("2000-02-10T18")
    inits = [np.datetime64("2000-01-05T00"),       # a stored time (used at td = 1)
             np.datetime64("2000-01-05T01"),       # between stored times: the next used one
             np.datetime64("2000-01-01T00"),       # before the first used time
             np.datetime64("2000-02-10T07"),       # the window runs past the end
             np.datetime64("2000-02-11T00")]       # after the last used time: nothing
    s = 4
    w = WindowIndex(TIMES, start, stop, td, inits, s)
    assert len(w) == R.length(0, s, inits) == 5
    got = w.frame_table(range(5))
    assert np.array_equal(got, _ref_table(TIMES, start, stop, td, s, inits, range(5)))
    used_times = TIMES[w.used]
    for i in (0, 1, 2):
        assert used_times[list(w.used).index(got[i, 0])] >= inits[i]
    assert got[1, 0] > got[0, 0] or td == 3
    assert got[2, 0] == w.used[0]
    assert (got[3] == -1).any() and got[3, 0] >= 0
    assert (got[4] == -1).all()
    with pytest.raises(IndexError):
        w.frame_table([5])


def test_channel_flattening_and_nan_fill_flags():
    """levels flatten into channels in the order the reference appends them (datasets.py:382-402); NaN fill: always for a
    variable without levels (:401), only under normalize for one with levels (:395-397), never for a prescribed one (:371)"""
    prog = {"z": [500, 850], "t2m": [], "u": [300]}
    levels = {"z": [300, 500, 850], "u": [300, 500]}
    for normalize in (False, True):
        p, q = channel_layout(prog, ["tisr", "sst"], levels, normalize)
        assert p == [("z", 500, normalize), ("z", 850, normalize), ("t2m", None, True), ("u", 300, normalize)]
        assert q == [("tisr", None, False), ("sst", None, False)]
    with pytest.raises(ValueError):
        channel_layout({"z": [700]}, [], levels, True)


def test_restatement_fills_like_the_flags():
    """the restatement's __getitem__ and channel_layout agree on where a NaN survives"""
    rng = np.random.default_rng(0)
    t = 6
    fields = {"z": rng.standard_normal((t, 2, 2, 3)).astype(np.float32), "t2m": rng.standard_normal((t, 2, 3)).astype(np.float32),
              "tisr": rng.standard_normal((t, 2, 3)).astype(np.float32)}
    for a in fields.values():
        a.reshape(-1)[::5] = np.nan
    levels = {"z": [500, 850]}
    stats = {"z": {"level": {500: {"mean": 0.1, "std": 2.0}, 850: {"mean": -0.3, "std": 0.5}}}, "t2m": {"mean": 0.2, "std": 1.5},
             "tisr": {"mean": 0.0, "std": 1.0}}
    for normalize in (False, True):
        _, pres, prog, tar = R.getitem(fields, levels, [0, 1, 2, 3], {"z": [850], "t2m": []}, ["tisr"], stats, normalize, 1)
        flags = [f for _, _, f in channel_layout({"z": [850], "t2m": []}, ["tisr"], levels, normalize)[0]]
        assert prog.shape == (3, 2, 2, 3) and tar.shape == (2, 2, 2, 3) and pres.shape == (3, 1, 2, 3)
        assert prog.dtype == np.float32 and pres.dtype == np.float32
        for c, f in enumerate(flags):
            assert np.isnan(prog[:, c]).any() == (not f)
        assert np.isnan(pres).any()


def test_header_and_signatures_name_the_dataset_entry_points():
    """tests/test_capi_cpu.py checks header and lib.SIGNATURES type by type; here: the four entry points exist in both"""
    from dlwp_benchmark_amd import lib as L

    lib = L.load()
    for name in ("dlwp_dataset_gather_f32", "dlwp_dataset_stats_f64", "dlwp_dataset_group_mean_f32", "dlwp_coarsen_mean_f32"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.dlwp_dataset_grid_blocks() > 0
    assert lib.dlwp_dataset_stats_workspace_bytes(3) > 0
