"""HEALPix face topology as gather tables (host side of dlwp_healpix_pad_f32 / dlwp_conv3x3_hpx_f32).

The reference pads every face with slices of its neighbours by running ~20 tensor ops per face per call
(utils/healpix.py:165-368).  The topology is static, so here it is evaluated ONCE, on cell indices instead of
values, into a table the kernels gather through: entry (a, b) per padded cell, a/b = face*H*W + pixel,
b = -1 for a plain copy, else the cell is the mean of both (the two corners an equatorial face has no
neighbour for, healpix.py:316-368).

Face order and orientation follow the reference (healpix.py:209-226): faces 0-3 north, 4-7 equator,
8-11 south; the neighbour of face f across each of its 8 borders is listed in `_NEIGHBOURS`, with the
quarter-turns that border crossing applies.
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

# per face group: border -> (neighbour face as a function of k = f % 4, quarter-turns counter-clockwise)
# borders: T top, B bottom, L left, R right and the four corners.  None = synthesised corner.
_N = lambda off: (lambda k: (k + off) % 4)
_E = lambda off: (lambda k: 4 + (k + off) % 4)
_S = lambda off: (lambda k: 8 + (k + off) % 4)
_NEIGHBOURS = (
    # north (healpix.py:209-212, pn :229-258)
    {"T": (_N(1), 1), "TL": (_N(2), 2), "L": (_N(3), -1), "BL": (_N(3), 0), "B": (_E(0), 0), "BR": (_S(0), 0),
     "R": (_E(1), 0), "TR": (_N(1), 0)},
    # equator (healpix.py:215-218, pe :260-283)
    {"T": (_N(0), 0), "TL": None, "L": (_N(3), 0), "BL": (_E(3), 0), "B": (_S(3), 0), "BR": None,
     "R": (_S(0), 0), "TR": (_E(1), 0)},
    # south (healpix.py:221-224, ps :285-314)
    {"T": (_E(1), 0), "TL": (_N(0), 0), "L": (_E(0), 0), "BL": (_S(3), 0), "B": (_S(3), 1), "BR": (_S(2), 2),
     "R": (_S(1), -1), "TR": (_S(1), 0)},
)


def _cells(face: int, h: int, w: int) -> np.ndarray:
    """[h, w, 2] descriptors (a, b) of one face's own cells."""
    a = face * h * w + np.arange(h * w, dtype=np.int64).reshape(h, w)
    return np.stack([a, np.full_like(a, -1)], axis=-1)


def _corner_from_two(first: np.ndarray, second: np.ndarray, p: int, top_left: bool) -> np.ndarray:
    """The p x p corner no face covers: off-diagonal cells continue the two adjacent faces, the diagonal is
    their mean (healpix.py:316-343 for top-left with (t, l), :345-368 for bottom-right with (b, r))."""
    out = np.full((p, p, 2), -1, dtype=np.int64)
    for i in range(p):
        if top_left:
            d = p - 1 - i                       # diagonal cell, counted from the inner corner outwards
            out[d, d] = (first[-i - 1, 0, 0], second[0, -i - 1, 0])
            if i:
                out[d, p - i:, 0] = first[-i - 1, :i, 0]
                out[p - i:, d, 0] = second[:i, -i - 1, 0]
        else:
            out[i, i] = (first[i, -1, 0], second[-1, i, 0])
            if i:
                out[:i, i, 0] = second[-i:, i, 0]
                out[i, :i, 0] = first[i, -i:, 0]
    return out


@functools.lru_cache(maxsize=32)
def pad_table(h: int, w: int, p: int) -> torch.Tensor:
    """int32 [12, (h+2p)*(w+2p), 2] gather table for HEALPixPadding(p) (CPU tensor; cache per shape)."""
    if h != w:
        raise ValueError("HEALPix faces are square")
    if not 0 < p <= h:
        raise ValueError(f"padding {p} does not fit a {h}x{w} face")
    table = np.empty((12, h + 2 * p, w + 2 * p, 2), dtype=np.int64)
    for f in range(12):
        rules, k = _NEIGHBOURS[f // 4], f % 4

        def nb(border):
            face_of, turns = rules[border]
            return np.rot90(_cells(face_of(k), h, w), turns, axes=(0, 1))

        pad = table[f]
        pad[p:-p, p:-p] = _cells(f, h, w)
        pad[:p, p:-p] = nb("T")[-p:, :]
        pad[-p:, p:-p] = nb("B")[:p, :]
        pad[p:-p, :p] = nb("L")[:, -p:]
        pad[p:-p, -p:] = nb("R")[:, :p]
        pad[-p:, :p] = nb("BL")[:p, -p:]
        pad[:p, -p:] = nb("TR")[-p:, :p]
        pad[:p, :p] = nb("TL")[-p:, -p:] if rules["TL"] else _corner_from_two(nb("T"), nb("L"), p, True)
        pad[-p:, -p:] = nb("BR")[:p, :p] if rules["BR"] else _corner_from_two(nb("B"), nb("R"), p, False)
    return torch.from_numpy(table.reshape(12, -1, 2).astype(np.int32))


_device_tables = {}


def device_table(h: int, w: int, p: int, device) -> torch.Tensor:
    key = (h, w, p, str(device))
    if key not in _device_tables:
        _device_tables[key] = pad_table(h, w, p).to(device).contiguous()
    return _device_tables[key]


class AdjointTable(NamedTuple):
    """CSR of the transpose of `pad_table`: for source cell s = face*h*w + pixel of one sample, entries
    indptr[s] .. indptr[s+1] list the padded positions q = face*(h+2p)*(w+2p) + padded pixel that read s, in increasing q,
    with their weight (1, or 0.5 for a synthesised corner, which is the mean of two cells)."""
    indptr: torch.Tensor     # int32 [12*h*w + 1]
    index: torch.Tensor      # int32 [nnz]
    weight: torch.Tensor     # float32 [nnz]


@functools.lru_cache(maxsize=32)
def pad_adjoint_table(h: int, w: int, p: int) -> AdjointTable:
    """The adjoint of HEALPixPadding(p) as a gather: dx[s] = sum over the entries of s of weight * dy[q] (CPU tensors)."""
    table = pad_table(h, w, p).reshape(-1, 2).numpy().astype(np.int64)
    q = np.arange(table.shape[0], dtype=np.int64)
    single = table[:, 1] < 0
    src = np.concatenate([table[:, 0], table[~single, 1]])
    pos = np.concatenate([q, q[~single]])
    wt = np.concatenate([np.where(single, 1.0, 0.5), np.full(int((~single).sum()), 0.5)])
    order = np.lexsort((pos, src))                  # by source cell, then by padded position
    src, pos, wt = src[order], pos[order], wt[order]
    indptr = np.zeros(12 * h * w + 1, dtype=np.int64)
    np.add.at(indptr, src + 1, 1)
    return AdjointTable(torch.from_numpy(np.cumsum(indptr).astype(np.int32)), torch.from_numpy(pos.astype(np.int32)),
                        torch.from_numpy(wt.astype(np.float32)))


_device_adjoints = {}


def device_adjoint_table(h: int, w: int, p: int, device) -> AdjointTable:
    key = (h, w, p, str(device))
    if key not in _device_adjoints:
        _device_adjoints[key] = AdjointTable(*(t.to(device).contiguous() for t in pad_adjoint_table(h, w, p)))
    return _device_adjoints[key]


# ---------------------------------------------------------------------------------------------------------------------
# HEALPix -> lat-lon remap (host side of dlwp_healpix_to_latlon_f32).  The reference remaps every rollout to lat-lon before
# it scores it (scripts/evaluate.py:79-116,298-303, scripts/train.py:430-441) by calling HEALPixRemap.hpx2ll
# (data/processing/healpix_mapping.py:372-404) once per plane on the host: a Python loop over the pixels, then reproject's
# bilinear interpolation.  The map is linear and fixed -- every lat-lon cell is a convex combination of at most four HEALPix
# cells -- so, like the padding, the geometry is evaluated ONCE, in float64, into a gather table.  Pixel centres and the
# interpolation rule are those of the HEALPix paper (Gorski et al. 2005, ApJ 622:759) and library (`get_interpol`).
# ---------------------------------------------------------------------------------------------------------------------
_JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)
_JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], dtype=np.int64)


def _check_nside(nside) -> int:
    n = int(nside)
    if n != nside or n < 2 or n & (n - 1):
        raise ValueError(f"nside must be a power of two >= 2 (the reference's bit interleave needs that), got {nside}")
    return n


@functools.lru_cache(maxsize=16)
def _cell_geometry(n: int):
    """(z, phi, ring index) of every cell [f, a, b], float64 / int64 [12, n, n].  Cell [f, a, b] of the reference's face
    layout (healpix_mapping.py:406-459: nested pixel (f, ix, iy) lands in hpx3d[f, ix, iy], then both face axes are flipped)
    is nested pixel (f, ix = n-1-a, iy = n-1-b)."""
    f = np.arange(12, dtype=np.int64)[:, None, None]
    ix = (n - 1 - np.arange(n, dtype=np.int64))[None, :, None]
    iy = (n - 1 - np.arange(n, dtype=np.int64))[None, None, :]
    jr = _JRLL[f] * n - ix - iy - 1                                # ring number, 1 .. 4n-1 from the north
    north, south = jr < n, jr > 3 * n
    nr = np.where(north, jr, np.where(south, 4 * n - jr, n))
    nrf = nr.astype(np.float64)
    z = np.where(north, 1.0 - nrf * nrf / (3.0 * n * n),
                 np.where(south, nrf * nrf / (3.0 * n * n) - 1.0, (2 * n - jr) * 2.0 / (3.0 * n)))
    kshift = np.where(north | south, 0, (jr - n) & 1)
    jp = (_JPLL[f] * nr + ix - iy + 1 + kshift) // 2               # pixel in the ring, wrapped into 1 .. 4 nr
    jp = np.where(jp > 4 * nr, jp - 4 * nr, jp)
    jp = np.where(jp < 1, jp + 4 * nr, jp)
    phi = (jp - (kshift + 1) * 0.5) * (0.5 * np.pi / nrf)
    start = np.where(north, 2 * nr * (nr - 1),
                     np.where(south, 12 * n * n - 2 * nr * (nr + 1), 2 * n * (n - 1) + (jr - n) * 4 * n))
    ring = start + jp - 1
    for a in (z, phi, ring):
        a.setflags(write=False)
    return z, phi, ring


def ring_index(nside: int) -> np.ndarray:
    """int64 [12, n, n]: the RING-scheme pixel number of cell [f, a, b] (a permutation of 0 .. 12 n^2 - 1)."""
    return _cell_geometry(_check_nside(nside))[2]


def cell_centres(nside: int):
    """(lat_deg, lon_deg), float64 [12, n, n]: where cell [f, a, b] of the reference's face layout sits on the sphere;
    [f, 0, 0] is the northern corner of face f."""
    z, phi, _ = _cell_geometry(_check_nside(nside))
    return np.degrees(np.arcsin(z)), np.degrees(phi)


def _as_f64(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))


def _ring_info(n: int, ring: np.ndarray):
    """(pixels in the ring, first RING index, theta of the ring, s) for ring numbers 1 .. 4n-1; pixel i of a ring is centred
    at (i + s/2) 2 pi / N."""
    north, south = ring < n, ring > 3 * n
    nr = np.where(north, ring, np.where(south, 4 * n - ring, n))
    nrf = nr.astype(np.float64)
    z = np.where(north, 1.0 - nrf * nrf / (3.0 * n * n),
                 np.where(south, nrf * nrf / (3.0 * n * n) - 1.0, (2 * n - ring) * 2.0 / (3.0 * n)))
    start = np.where(north, 2 * nr * (nr - 1),
                     np.where(south, 12 * n * n - 2 * nr * (nr + 1), 2 * n * (n - 1) + (ring - n) * 4 * n))
    s = np.where(north | south, 1, 1 - ((ring - n) & 1))
    return 4 * nr, start, np.arccos(z), s


def interp_weights(nside: int, lats_deg, lons_deg):
    """The HEALPix library's bilinear interpolation (`get_interpol`, healpy `get_interp_weights`: what reproject_from_healpix
    applies at its default order) for the H x W grid of targets (lats_deg[j], lons_deg[i]), target q = j W + i:
    (cell int64 [H W, 4], weight float64 [H W, 4]) with cell = face n^2 + a n + b in the layout of `cell_centres`.  Taps 0, 1
    lie on the ring above the target, 2, 3 on the ring below; beyond the first and last ring the missing pair is the ring's
    four pixels (the two listed taps, turned by half the ring) at a quarter of the remaining weight each."""
    n = _check_nside(nside)
    lats, lons = _as_f64(lats_deg), _as_f64(lons_deg)
    if lats.size == 0 or lons.size == 0 or not (np.all(np.abs(lats) <= 90.0) and np.all(np.isfinite(lons))):
        raise ValueError("latitudes must lie in [-90, 90] and longitudes be finite, at least one of each")
    theta = np.repeat(np.radians(90.0 - lats), lons.size)
    phi = np.tile(np.radians(np.mod(lons, 360.0)), lats.size)
    z = np.cos(theta)
    az = np.abs(z)
    cap = np.floor(n * np.sqrt(3.0 * (1.0 - az))).astype(np.int64)
    ir1 = np.where(az <= 2.0 / 3.0, np.floor(n * (2.0 - 1.5 * z)).astype(np.int64), np.where(z > 0, cap, 4 * n - cap - 1))
    ir2 = ir1 + 1
    npix = 12 * n * n
    pix = np.zeros((theta.size, 4), dtype=np.int64)
    wgt = np.zeros((theta.size, 4), dtype=np.float64)
    th = [None, None]
    for k, ir in enumerate((ir1, ir2)):
        ok = (ir >= 1) & (ir <= 4 * n - 1)
        cnt, start, th[k], s = _ring_info(n, np.clip(ir, 1, 4 * n - 1))
        t = phi * cnt / (2.0 * np.pi) - 0.5 * s
        i1 = np.floor(t).astype(np.int64)
        w = t - i1
        i2 = i1 + 1
        i1 = np.where(i1 < 0, i1 + cnt, np.where(i1 >= cnt, i1 - cnt, i1))
        i2 = np.where(i2 >= cnt, i2 - cnt, i2)
        pix[:, 2 * k], pix[:, 2 * k + 1] = np.where(ok, start + i1, 0), np.where(ok, start + i2, 0)
        wgt[:, 2 * k], wgt[:, 2 * k + 1] = np.where(ok, 1.0 - w, 0.0), np.where(ok, w, 0.0)
    top, bottom = ir1 == 0, ir2 == 4 * n
    mid = ~(top | bottom)
    wt = np.where(mid, (theta - th[0]) / np.where(mid, th[1] - th[0], 1.0), 0.0)
    wt = np.where(top, theta / th[1], wt)
    wt = np.where(bottom, (theta - th[0]) / (np.pi - th[0]), wt)
    wgt[:, :2] *= (1.0 - wt)[:, None]
    wgt[:, 2:] *= wt[:, None]
    fac = np.where(top, (1.0 - wt) * 0.25, 0.0)                    # above the first ring: the rest goes to its four pixels
    wgt[:, 0] = np.where(top, fac, wgt[:, 0])
    wgt[:, 1] = np.where(top, fac, wgt[:, 1])
    wgt[:, 2] += fac
    wgt[:, 3] += fac
    pix[:, 0] = np.where(top, (pix[:, 2] + 2) & 3, pix[:, 0])
    pix[:, 1] = np.where(top, (pix[:, 3] + 2) & 3, pix[:, 1])
    fac = np.where(bottom, wt * 0.25, 0.0)                         # below the last ring: the mirror image
    wgt[:, 0] += fac
    wgt[:, 1] += fac
    wgt[:, 2] = np.where(bottom, fac, wgt[:, 2])
    wgt[:, 3] = np.where(bottom, fac, wgt[:, 3])
    pix[:, 2] = np.where(bottom, ((pix[:, 0] + 2) & 3) + npix - 4, pix[:, 2])
    pix[:, 3] = np.where(bottom, ((pix[:, 1] + 2) & 3) + npix - 4, pix[:, 3])
    if pix.min() < 0 or pix.max() >= npix:
        raise ValueError("HEALPix interpolation produced a pixel outside the map")
    cell_of_ring = np.empty(npix, dtype=np.int64)
    cell_of_ring[ring_index(n).reshape(-1)] = np.arange(npix, dtype=np.int64)
    return cell_of_ring[pix], wgt


class LatLonTable(NamedTuple):
    """Gather table of the HEALPix -> lat-lon remap: y[q] = sum_t weight[q, t] * x[index[q, t]] over the 12 n^2 cells of one
    plane, q = j W + i (see `interp_weights`)."""
    index: torch.Tensor      # int32 [H*W, 4], face*n*n + a*n + b
    weight: torch.Tensor     # float32 [H*W, 4]


_latlon_tables = {}


def latlon_table(nside: int, lats_deg, lons_deg) -> LatLonTable:
    """`interp_weights` as CPU tensors for the kernel: weights computed in float64 and rounded once to float32, every index
    checked against 12 n^2 here (the kernel does not).  Cached per argument set."""
    n = _check_nside(nside)
    lats, lons = _as_f64(lats_deg), _as_f64(lons_deg)
    key = (n, lats.tobytes(), lons.tobytes())
    if key not in _latlon_tables:
        cell, wgt = interp_weights(n, lats, lons)
        if cell.min() < 0 or cell.max() >= 12 * n * n:
            raise ValueError("remap table index outside the 12 n^2 cells of a plane")
        if len(_latlon_tables) >= 32:
            _latlon_tables.pop(next(iter(_latlon_tables)))
        _latlon_tables[key] = LatLonTable(torch.from_numpy(cell.astype(np.int32)), torch.from_numpy(wgt.astype(np.float32)))
    return _latlon_tables[key]


def reference_grid(latitudes: int, longitudes: int):
    """(lats_deg, lons_deg), float64: the target grid HEALPixRemap.hpx2ll produces, read from its WCS header
    (healpix_mapping.py:109-123: CRVAL1 = 179 at CRPIX1 = longitudes / 2, CDELT = 360 / longitudes on both axes), north
    first.  At 180 x 360 that is lon 0 .. 359 and lat 89.5 .. -89.5; at 32 x 64 the header's 179 puts lon_0 at 4.625 -- a
    quirk of the reference that belongs here and nowhere else (the metric classes take explicit arrays)."""
    latitudes, longitudes = int(latitudes), int(longitudes)
    res = 360.0 / longitudes
    lons = np.mod(179.0 + res * (np.arange(longitudes, dtype=np.float64) + 1.0 - longitudes / 2.0), 360.0)
    lats = res * ((latitudes - 1) / 2.0 - np.arange(latitudes, dtype=np.float64))
    return lats, lons


_device_latlon_tables = {}


def device_latlon_table(nside: int, lats_deg, lons_deg, device) -> LatLonTable:
    lats, lons = _as_f64(lats_deg), _as_f64(lons_deg)
    key = (int(nside), lats.tobytes(), lons.tobytes(), str(device))
    if key not in _device_latlon_tables:
        _device_latlon_tables[key] = LatLonTable(*(t.to(device).contiguous() for t in latlon_table(nside, lats, lons)))
    return _device_latlon_tables[key]
