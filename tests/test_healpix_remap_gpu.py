"""HEALPix -> lat-lon remap on the device (dlwp_healpix_to_latlon_f32, csrc/healpix_remap.hip) and the metric classes on HEALPix
rollouts.

The kernel is compared with a float64 numpy application of the SAME float32 table, written here.  Per output the kernel rounds
four products and three sums: |err| <= 5 * 2^-24 * sum_i w_i |x_i| ~ 3e-7 max|x| (the weights are >= 0 and sum to 1); the
tolerance is 1e-6 max|x|, that bound with 3x headroom.  Parity with the reference's HEALPixRemap.hpx2ll is not pinned by a fixture
(healpy / reproject / astropy are not available where fixtures are made): the table itself is pinned by
tests/test_healpix_remap_cpu.py.
"""
import numpy as np
import pytest
import torch

from dlwp_benchmark_amd import healpix as H
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd.lib import DlwpError
from dlwp_benchmark_amd.metrics import RolloutMetrics, ZonalSpectrumMetrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _grid(name):
    if name == "poles_seam_3x5":
        return np.array([90.0, 10.0, -90.0]), np.array([0.0, 77.0, 180.0, 300.0, 360.0])
    if name == "4x8":
        return 67.5 - 45.0 * np.arange(4.0), 22.5 + 45.0 * np.arange(8.0)
    if name == "ref32x64":
        return H.reference_grid(32, 64)
    if name == "irregular_5x7":
        return np.array([88.9, 60.0, 41.81, 0.0, -71.2]), np.array([0.1, 44.9, 45.0, 123.4, 200.0, 270.0, 355.5])
    if name == "8x16":
        return 78.75 - 22.5 * np.arange(8.0), 11.25 + 22.5 * np.arange(16.0)
    if name == "ref180x360":
        return H.reference_grid(180, 360)
    raise KeyError(name)


def _reference(x: np.ndarray, table) -> np.ndarray:
    """float64: y[p, q] = sum_t weight[q, t] * x[p, index[q, t]] with the float32 table's values"""
    idx = table.index.numpy().astype(np.int64)
    w = table.weight.numpy().astype(np.float64)
    flat = x.reshape(x.shape[0], -1).astype(np.float64)
    y = np.zeros((flat.shape[0], idx.shape[0]), dtype=np.float64)
    for t in range(4):
        y += w[:, t] * flat[:, idx[:, t]]
    return y


# (nside, grid, planes).  One kernel, no dispatch: a workgroup takes 1024 consecutive cells (a thread four of them, 256 apart)
# and 16 planes, walked two at a time, then singly.  Poles and the seam on 15 cells; a plane count past any 16-bit grid axis;
# the reference's grid (two workgroups along the cells); a cell count that fills no wave with a plane count that ends on a
# one-plane block; a plane larger than LDS; several workgroups along the cells, the last with threads that hold one, two or no
# cell (64800 = 63 * 1024 + 288) and a last block of 7 planes (three pairs, then one).
CASES = [(2, "poles_seam_3x5", 1), (2, "4x8", 70001), (8, "ref32x64", 3), (8, "irregular_5x7", 33), (64, "8x16", 2),
         (16, "ref180x360", 23)]


@pytest.mark.parametrize("nside,grid,planes", CASES, ids=[f"n{n}-{g}-p{p}" for n, g, p in CASES])
def test_kernel_against_float64_reference(nside, grid, planes):
    lats, lons = _grid(grid)
    gen = torch.Generator().manual_seed(1000 * nside + planes)
    x = 3.0 * torch.randn(planes, 12, nside, nside, generator=gen) + 0.5
    table = H.latlon_table(nside, lats, lons)
    assert int(table.index.min()) >= 0 and int(table.index.max()) < 12 * nside * nside
    y = ops.healpix_to_latlon(x.to(DEV), lats, lons)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (planes, len(lats), len(lons)) and y.dtype == torch.float32
    want = _reference(x.numpy(), table)
    err = float(np.abs(y.cpu().numpy().reshape(planes, -1).astype(np.float64) - want).max())
    bound = 1e-6 * float(x.abs().max())
    print(f"nside {nside} {grid} planes {planes}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_non_contiguous_view_and_leading_dimensions():
    lats, lons = H.reference_grid(32, 64)
    gen = torch.Generator().manual_seed(7)
    base = torch.randn(3, 2, 2, 12, 8, 8, generator=gen).to(DEV)
    x = base.permute(1, 0, 2, 3, 4, 5)                     # [2, 3, 2, 12, 8, 8], not contiguous
    assert tuple(x.shape) == (2, 3, 2, 12, 8, 8) and not x.is_contiguous()
    y = ops.healpix_to_latlon(x, lats, lons)
    assert tuple(y.shape) == (2, 3, 2, 32, 64)
    want = _reference(x.cpu().numpy().reshape(12, 12, 8, 8), H.latlon_table(8, lats, lons)).reshape(2, 3, 2, 32, 64)
    assert float(np.abs(y.cpu().numpy().astype(np.float64) - want).max()) <= 1e-6 * float(x.abs().max())
    assert torch.equal(y, ops.healpix_to_latlon(x.contiguous(), lats, lons))


def test_nan_cell_reaches_exactly_the_outputs_that_tap_it():
    lats, lons = H.reference_grid(32, 64)
    table = H.latlon_table(8, lats, lons)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 12, 8, 8, generator=gen)
    cell = 5 * 64 + 3 * 8 + 4
    x.view(2, -1)[1, cell] = float("nan")
    y = ops.healpix_to_latlon(x.to(DEV), lats, lons).cpu().reshape(2, -1)
    taps = (table.index == cell).any(dim=1)                # a tap of weight zero counts: 0 * NaN is NaN, as in numpy
    assert 0 < int(taps.sum()) < taps.numel()
    assert not torch.isnan(y[0]).any()
    assert torch.equal(torch.isnan(y[1]), taps)
    assert np.array_equal(np.isnan(_reference(x.numpy(), table)[1]), taps.numpy())


def _hpx_rollouts():
    gen = torch.Generator().manual_seed(23)
    target = torch.randn(3, 2, 2, 12, 8, 8, generator=gen)
    out = 1.5 * target + 0.3 * torch.randn(3, 2, 2, 12, 8, 8, generator=gen)      # correlated, and 2.25x the energy
    return out.to(DEV), target.to(DEV)


def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("one_sample_chunks", [False, True], ids=["one_chunk", "chunk_per_sample"])
def test_metric_classes_take_healpix_rollouts(one_sample_chunks):
    """6-D input equals the same classes on the pre-remapped 5-D tensors: the per-workgroup fp32 partial sums are the same, only
    the order of the fp64 additions differs."""
    lats, lons = H.reference_grid(32, 64)
    out, target = _hpx_rollouts()
    gen = torch.Generator().manual_seed(29)
    std = torch.tensor([2.0, 0.5])
    clim = 0.2 * torch.randn(2, 2, 32, 64, generator=gen)
    per_sample = 2 * 2 * 32 * 64 * 4 * 2                    # bytes of one sample of out and of target on the lat-lon grid
    kw = {"max_workspace_bytes": per_sample} if one_sample_chunks else {}
    out_ll, target_ll = ops.healpix_to_latlon(out, lats, lons), ops.healpix_to_latlon(target, lats, lons)

    plain = RolloutMetrics(torch.from_numpy(lats), std=std, climatology=clim)
    want = plain(out_ll, target_ll)
    hpx = RolloutMetrics(torch.from_numpy(lats), std=std, climatology=clim, lons_deg=lons, **kw)
    got = hpx(out, target)
    assert tuple(got["rmse"].shape) == (2, 2) and got["acc"] is not None
    _close(got["rmse"], want["rmse"])
    _close(got["acc"], want["acc"])
    assert hpx._remap_ws[str(out.device)].numel() * 4 == (per_sample if one_sample_chunks else 3 * per_sample)
    # running sums: added to what `into` holds
    running = plain.sums(out_ll, target_ll)
    again = hpx.sums(out, target, into=running.clone())
    _close(again, 2 * running)

    zplain = ZonalSpectrumMetrics(torch.from_numpy(lats))
    zwant = zplain(out_ll, target_ll)
    zhpx = ZonalSpectrumMetrics(torch.from_numpy(lats), lons_deg=torch.from_numpy(lons), **kw)
    zgot = zhpx(out, target)
    for key in ("energy_pred", "energy_true", "log_ratio", "melr"):
        assert zgot[key].shape == zwant[key].shape
        _close(zgot[key], zwant[key])
    assert float(zwant["melr"].abs().min()) > 0.1
    # 5-D input through a class that has longitudes is the plain path, bit for bit
    assert torch.equal(hpx.sums(out_ll, target_ll), plain.sums(out_ll, target_ll))
    torch.cuda.synchronize()


def test_errors():
    lats, lons = H.reference_grid(32, 64)
    out, target = _hpx_rollouts()
    with pytest.raises(DlwpError, match="lons_deg"):
        RolloutMetrics(torch.from_numpy(lats)).sums(out, target)
    with pytest.raises(DlwpError, match="lons_deg"):
        ZonalSpectrumMetrics(torch.from_numpy(lats)).sums(out, target)
    with pytest.raises(DlwpError, match="12"):
        ops.healpix_to_latlon(torch.zeros(2, 11, 8, 8, device=DEV), lats, lons)
    with pytest.raises(DlwpError, match="square"):
        ops.healpix_to_latlon(torch.zeros(2, 12, 8, 4, device=DEV), lats, lons)
    with pytest.raises(DlwpError, match="power of two"):
        ops.healpix_to_latlon(torch.zeros(2, 12, 6, 6, device=DEV), lats, lons)
    with pytest.raises(ValueError, match="power of two"):
        H.latlon_table(6, lats, lons)
    with pytest.raises(DlwpError, match="no CPU fallback"):
        ops.healpix_to_latlon(torch.zeros(2, 12, 8, 8), lats, lons)
    with pytest.raises(DlwpError, match="max_workspace_bytes"):
        RolloutMetrics(torch.from_numpy(lats), lons_deg=lons, max_workspace_bytes=1024).sums(out, target)
    with pytest.raises(DlwpError, match="target shape"):
        RolloutMetrics(torch.from_numpy(lats), lons_deg=lons).sums(out, target[:2])
