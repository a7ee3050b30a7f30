"""Host geometry of the HEALPix -> lat-lon remap (dlwp_benchmark_amd/healpix.py: cell_centres, latlon_table, reference_grid).

Parity with the reference's HEALPixRemap.hpx2ll is NOT pinned by a fixture: healpy, reproject and astropy are not installed where
the fixtures are made.  What pins the table instead: the face layout is tied to the padding table (which IS pinned bit for bit
against the reference's HEALPixPadding), the orientation to the published face positions, the interpolation to its own algebra
(convex rows, exact at cell centres) and to analytic fields whose error bounds separate a correct table from a shift by one cell
or a mirror.
"""
import numpy as np
import pytest

from dlwp_benchmark_amd import healpix as H


def _unit(lat_deg, lon_deg):
    la, lo = np.radians(lat_deg), np.radians(lon_deg)
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=-1)


def _angle(u, v):
    """great-circle distance of unit vectors, accurate for small and large angles"""
    return 2.0 * np.arcsin(np.clip(0.5 * np.linalg.norm(u - v, axis=-1), 0.0, 1.0))


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_layout_is_a_permutation_and_agrees_with_the_padding_table(n):
    ring = H.ring_index(n)
    assert ring.shape == (12, n, n)
    assert np.array_equal(np.sort(ring.reshape(-1)), np.arange(12 * n * n))
    lat, lon = H.cell_centres(n)
    assert lat.shape == lon.shape == (12, n, n) and lat.dtype == lon.dtype == np.float64
    xyz = _unit(lat, lon).reshape(-1, 3)
    side = np.sqrt(4.0 * np.pi / (12 * n * n))
    # the four edge neighbours of every cell under the padding table (face borders included): pad 1, the cells above, below,
    # left and right of the interior; none of these is a synthesised corner
    pad = H.pad_table(n, n, 1).numpy().reshape(12, n + 2, n + 2, 2).astype(np.int64)
    own = pad[:, 1:-1, 1:-1, 0].reshape(-1)
    assert np.array_equal(own, np.arange(12 * n * n))
    worst = 0.0
    for nb in (pad[:, :-2, 1:-1], pad[:, 2:, 1:-1], pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]):
        assert (nb[..., 1] < 0).all()
        d = _angle(xyz[own], xyz[nb[..., 0].reshape(-1)])
        worst = max(worst, float(d.max()) / side)
    print(f"n={n}: largest edge-neighbour distance {worst:.3f} cell sides")
    assert worst <= 1.5
    # no two distinct cells closer than 0.81 of a side
    gram = xyz @ xyz.T
    np.fill_diagonal(gram, -1.0)
    nearest = np.arccos(np.clip(gram.max(), -1.0, 1.0)) / side
    print(f"n={n}: smallest distance between two cells {nearest:.3f} cell sides")
    assert nearest >= 0.81


@pytest.mark.parametrize("n", [2, 8])
def test_orientation(n):
    lat, lon = H.cell_centres(n)
    for f in range(12):
        assert lat[f, 0, 0] == lat[f].max() and (lat[f].reshape(-1)[1:] < lat[f, 0, 0]).all()
    assert (lat[:4].mean(axis=(1, 2)) > 0).all() and (lat[8:].mean(axis=(1, 2)) < 0).all()
    assert np.allclose(lat[4:8].mean(axis=(1, 2)), 0.0, atol=1e-12)
    centre = _unit(lat, lon).mean(axis=(1, 2))
    centre_lon = np.degrees(np.arctan2(centre[:, 1], centre[:, 0])) % 360.0
    for k in range(4):
        assert abs(centre_lon[k] - (45 + 90 * k)) < 1e-9
        assert abs(centre_lon[8 + k] - (45 + 90 * k)) < 1e-9
        assert min(abs(centre_lon[4 + k] - 90 * k), abs(centre_lon[4 + k] - 90 * k - 360), abs(centre_lon[4 + k] - 90 * k + 360)) < 1e-9


_GRIDS = {
    "ref32x64": lambda: H.reference_grid(32, 64),
    "poles_and_seam": lambda: (np.array([90.0, 37.3, -90.0]), np.array([0.0, 90.0, 181.7, 359.99, 360.0])),
    "irregular": lambda: (np.array([88.9, 60.0, 41.81, 0.0, -71.2]), np.array([0.1, 44.9, 45.0, 123.4, 200.0, 270.0, 355.5])),
}


@pytest.mark.parametrize("grid", sorted(_GRIDS))
@pytest.mark.parametrize("n", [2, 8, 16])
def test_table_rows_are_convex(n, grid):
    lats, lons = _GRIDS[grid]()
    cell, w64 = H.interp_weights(n, lats, lons)
    cells = len(lats) * len(lons)
    assert cell.shape == w64.shape == (cells, 4) and w64.dtype == np.float64
    assert cell.min() >= 0 and cell.max() < 12 * n * n
    assert (w64 >= 0).all()
    assert np.abs(w64.sum(axis=1) - 1.0).max() <= 1e-15
    t = H.latlon_table(n, lats, lons)
    assert str(t.index.dtype) == "torch.int32" and str(t.weight.dtype) == "torch.float32"
    assert tuple(t.index.shape) == tuple(t.weight.shape) == (cells, 4)
    assert np.array_equal(t.index.numpy(), cell.astype(np.int32))
    assert np.array_equal(t.weight.numpy(), w64.astype(np.float32))            # rounded once
    assert np.abs(t.weight.numpy().astype(np.float64).sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -24
    assert H.latlon_table(n, lats, lons) is t                                   # cached per argument set


@pytest.mark.parametrize("n", [2, 8])
def test_exact_at_cell_centres(n):
    lat, lon = H.cell_centres(n)
    # one target per cell; the builder takes an outer product of latitudes and longitudes, so the cells go ring by ring
    for la in np.unique(lat):
        sel = np.flatnonzero(lat.reshape(-1) == la)
        cell, w = H.interp_weights(n, np.array([la]), lon.reshape(-1)[sel])
        for row, c in enumerate(sel):
            on = float(w[row][cell[row] == c].sum())
            assert abs(on - 1.0) <= 1e-12, (n, c, cell[row], w[row])


def _apply64(cell, w, field):
    return (w * field.reshape(-1)[cell]).sum(axis=1)


@pytest.mark.parametrize("shape", [(32, 64), (180, 360)])
@pytest.mark.parametrize("n,bound", [(8, 0.05), (16, 0.03)])
def test_degree_one_harmonics(n, bound, shape):
    """x, y, z of the unit vector sampled at the cell centres, remapped in float64, against the field at the targets.  A table
    shifted by one 5.625 degree cell errs by 0.098, any mirror by about 1."""
    lats, lons = H.reference_grid(*shape)
    cell, w = H.interp_weights(n, lats, lons)
    src = _unit(*H.cell_centres(n))                                   # [12, n, n, 3]
    want = _unit(np.repeat(lats, len(lons)), np.tile(lons, len(lats)))
    for comp in range(3):
        err = float(np.abs(_apply64(cell, w, src[..., comp]) - want[:, comp]).max())
        print(f"n={n} grid {shape} component {'xyz'[comp]}: max error {err:.4f}")
        assert err <= bound, (n, shape, comp, err)


def test_reference_grid():
    lats, lons = H.reference_grid(180, 360)
    assert lats.shape == (180,) and lons.shape == (360,)
    assert np.array_equal(lons, np.arange(360.0))
    assert np.array_equal(lats, 89.5 - np.arange(180.0))
    lats, lons = H.reference_grid(32, 64)
    assert lons[0] == 4.625 and lats[0] == 5.625 * 15.5 and lats[-1] == -5.625 * 15.5
    assert np.allclose(np.diff(lons) % 360.0, 5.625)


@pytest.mark.parametrize("nside", [0, 1, 3, 6, 12])
def test_nside_must_be_a_power_of_two(nside):
    with pytest.raises(ValueError, match="power of two"):
        H.cell_centres(nside)
    with pytest.raises(ValueError, match="power of two"):
        H.latlon_table(nside, [0.0], [0.0])
