"""ops.sph_power_sums / metrics.SphericalSpectrumMetrics (csrc/sph_power.hip) against the float64 restatement of
tests/sph_spectrum_ref.py.

Tolerance rule (per case and per quantity): the error of the float32 numpy restatement (the SAME fp32
tables as the device, fp32 accumulation, the difference formed in the field domain) against float64 is computed; the kernel is
allowed 8 x that error -- its summation order differs -- with a floor of 1e-6.  The error norm of a quantity is, per (k, c),
max_l |delta| / max_l |reference|, and the worst (k, c) counts; for the cross spectrum the denominator is
sqrt(max_l P0 max_l P1), since the cross spectrum of independent fields is near zero.  Every figure is printed before it is
asserted; the measured ones stand in DESIGN.md section 36.  Float64 tables: the independent ones of the restatement up to
lmax 33, sphere.py's float64 tables above.
"""
import numpy as np
import pytest
import torch

import sht_ref as R
import sph_spectrum_ref as SR
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd import sphere as S
from dlwp_benchmark_amd.lib import DlwpError
from dlwp_benchmark_amd.metrics import SphericalSpectrumMetrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LG, EQ, CE = "legendre-gauss", "equiangular", "equiangular-centred"
NAMES = ("power(out)", "power(target)", "power(out - target)", "cross")


def _tables64(grid, nlat, lmax, mmax):
    if max(lmax, mmax) <= R.MAX_INDEPENDENT_L:
        return SR.tables(grid, nlat, lmax, mmax)
    theta, w = S.quadrature(grid, nlat)
    return S.legendre(mmax, lmax, theta), w


def _errors(got, want):
    """the error norm of each of the four quantities: [4], the worst (k, c) of each"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    peak = np.abs(want).max(-1)                                         # [4, K, C]
    den = np.stack([peak[0], peak[1], peak[2], np.sqrt(peak[0] * peak[1])])
    return (np.abs(got - want).max(-1) / den).max((-2, -1))


def _references(out, tar, grid, lmax, mmax, k_slice=None):
    """(float64 sums, float32 restatement sums) of float32 numpy inputs [B, K, C, nlat, nlon], computed k_slice lead steps at a
    time where the whole batch would be large"""
    nlat, nlon = out.shape[-2:]
    p, w = _tables64(grid, nlat, lmax, mmax)
    wleg32, _ = S.tables_f32(grid, nlat, lmax, mmax)
    tw32 = S.twiddles(nlon).astype(np.float32)
    k = out.shape[1]
    step = k if k_slice is None else k_slice
    want = np.concatenate([SR.sums(out[:, a:a + step], tar[:, a:a + step], p, w) for a in range(0, k, step)], axis=1)
    f32 = np.concatenate([SR.sums_f32(out[:, a:a + step], tar[:, a:a + step], wleg32, tw32) for a in range(0, k, step)], axis=1)
    return want, f32


def _check(label, got, want, f32, quantities=range(4)):
    err, e32 = _errors(got, want), _errors(f32, want)
    for q in quantities:
        print(f"sph_power {label} {NAMES[q]}: kernel {err[q]:.3e}, float32 restatement {e32[q]:.3e}")
    for q in quantities:
        assert err[q] <= max(8.0 * e32[q], 1e-6), (label, NAMES[q])


def _pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


# (grid, nlat, nlon, lmax, mmax, (B, K, C)): the smallest; units that are no multiple of a workgroup's share; a nlon that is no
# power of two with min(l, mmax - 1); the new grid; odd nlat; the Nyquist column (f = 1, imaginary part dropped); the
# evaluation grid; several m tiles and row chunks, so that the partials of a unit span tiles; the corner of the envelope.
CASES = [(LG, 8, 16, 8, 8, (1, 1, 1)), (LG, 8, 16, 8, 8, (3, 2, 2)), (LG, 12, 20, 7, 5, (2, 1, 3)), (CE, 8, 16, 4, 4, (2, 2, 1)),
         (EQ, 9, 16, 4, 4, (1, 1, 2)), (LG, 12, 16, 10, 9, (2, 1, 1)), (CE, 32, 64, 32, 32, (4, 3, 2)),
         (LG, 64, 128, 64, 64, (2, 1, 2)), (LG, 256, 512, 256, 257, (1, 1, 1))]
IDS = [f"{g[:2] if g != CE else 'ce'}-{a}x{b}-l{l}-m{m}-{'x'.join(map(str, u))}" for g, a, b, l, m, u in CASES]


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax,bkc", CASES, ids=IDS)
def test_sums_against_float64(grid, nlat, nlon, lmax, mmax, bkc):
    out, tar = _pair(bkc + (nlat, nlon), 21)
    want, f32 = _references(out, tar, grid, lmax, mmax)
    od, td = _dev(out), _dev(tar)
    got = ops.sph_power_sums(od, td, grid, lmax, mmax)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4,) + bkc[1:] + (lmax,)
    again = ops.sph_power_sums(od, td, grid, lmax, mmax)
    _check(f"{grid} {nlat}x{nlon} l{lmax} m{mmax} {bkc}", got.cpu().numpy(), want, f32)
    assert torch.equal(got, again)                                      # a call repeated gives the same bits


def test_seventy_thousand_units_on_the_grid_axis():
    """B K C = 70007 passes the 65535 of a 16-bit grid axis; the float64 reference is computed in slices"""
    grid, nlat, nlon, lmax, bkc = LG, 8, 16, 8, (7, 73, 137)
    out, tar = _pair(bkc + (nlat, nlon), 22)
    want, f32 = _references(out, tar, grid, lmax, lmax, k_slice=8)
    got = ops.sph_power_sums(_dev(out), _dev(tar), grid, lmax, lmax)
    _check(f"{grid} {nlat}x{nlon} l{lmax} {bkc}", got.cpu().numpy(), want, f32)


def test_error_spectrum_of_a_near_perfect_forecast():
    """target = out + 1e-3 noise: the error spectrum keeps its accuracy because the difference is formed in the field domain
    (a kernel that subtracted coefficients would carry the transforms' rounding relative to the FIELD, a thousand times the
    error's size, and fail here)"""
    grid, nlat, nlon, lmax = LG, 32, 64, 32
    rng = np.random.default_rng(23)
    out = rng.standard_normal((2, 2, 2, nlat, nlon)).astype(np.float32)
    tar = (out + np.float32(1e-3) * rng.standard_normal(out.shape).astype(np.float32)).astype(np.float32)
    want, f32 = _references(out, tar, grid, lmax, lmax)
    got = ops.sph_power_sums(_dev(out), _dev(tar), grid, lmax, lmax)
    _check("near-perfect lg 32x64 l32", got.cpu().numpy(), want, f32)


@pytest.mark.parametrize("cut", [1, 2])
def test_a_batch_cut_anywhere_gives_the_bits_of_the_one_shot_call(cut):
    for grid, nlat, nlon, lmax, kc in ((LG, 8, 16, 8, (1, 1)), (LG, 64, 128, 64, (2, 1))):     # one m tile; several
        out, tar = (_dev(a) for a in _pair((3,) + kc + (nlat, nlon), 24))
        whole = ops.sph_power_sums(out, tar, grid, lmax)
        run = torch.zeros_like(whole)
        assert ops.sph_power_sums(out[:cut], tar[:cut], grid, lmax, into=run) is run
        ops.sph_power_sums(out[cut:], tar[cut:], grid, lmax, into=run)
        assert torch.equal(run, whole), (grid, nlat, cut)
        first = ops.sph_power_sums(out[:cut], tar[:cut], grid, lmax)     # the chain may also start from the first part's sums
        ops.sph_power_sums(out[cut:], tar[cut:], grid, lmax, into=first)
        assert torch.equal(first, whole)


def test_arguments_are_checked():
    x = torch.zeros(2, 1, 1, 8, 16, device=DEV)
    good = torch.zeros(4, 1, 1, 8, dtype=torch.float64, device=DEV)
    ops.sph_power_sums(x, x, LG, into=good)
    with pytest.raises(DlwpError, match="double"):
        ops.sph_power_sums(x, x, LG, into=torch.zeros(4, 1, 1, 7, dtype=torch.float64, device=DEV))      # shape
    with pytest.raises(DlwpError, match="double"):
        ops.sph_power_sums(x, x, LG, into=torch.zeros(4, 1, 1, 8, dtype=torch.float32, device=DEV))      # dtype
    with pytest.raises(DlwpError, match="MI355X"):
        ops.sph_power_sums(x, x, LG, into=torch.zeros(4, 1, 1, 8, dtype=torch.float64))                  # device
    with pytest.raises(DlwpError, match="supported range"):
        ops.sph_power_sums(x, x, LG, 9, 8)                                                               # lmax > nlat
    with pytest.raises(DlwpError, match="supported range"):
        ops.sph_power_sums(torch.zeros(1, 1, 1, 8, 15, device=DEV), torch.zeros(1, 1, 1, 8, 15, device=DEV), LG)   # odd nlon
    with pytest.raises(DlwpError, match="unknown grid"):
        ops.sph_power_sums(x, x, "equiangular-centered")
    with pytest.raises(DlwpError, match="no CPU fallback"):
        ops.sph_power_sums(x.cpu(), x.cpu(), LG)
    with pytest.raises(DlwpError, match="target shape"):
        ops.sph_power_sums(x, x[:1], LG)
    with pytest.raises(DlwpError, match=r"\[B, K, C, nlat, nlon\]"):
        ops.sph_power_sums(x[0], x[0], LG)


def test_the_library_refuses_what_the_wrapper_would():
    """the C entry point's own envelope and workspace checks (the wrapper refuses these shapes before it launches)"""
    from dlwp_benchmark_amd import lib

    L = lib.load()
    assert L.dlwp_sph_power_workspace_bytes(1, 1, 1, 8, 16, 9, 8) == 0
    assert L.dlwp_sph_power_workspace_bytes(2, 3, 5, 8, 16, 8, 8) == 8 * 4 * 30 * 8
    tab = S.device_tables(LG, 8, 16, 8, 8, torch.device(DEV))
    x = torch.zeros(1, 1, 1, 8, 16, device=DEV)
    sums = torch.zeros(4, 1, 1, 8, dtype=torch.float64, device=DEV)
    ws = torch.empty(4096, dtype=torch.uint8, device=DEV)
    with pytest.raises(DlwpError) as e:
        lib.launch("dlwp_sph_power_sums_f32", x.device, x, x, tab.wleg, tab.tw, sums, 1, 1, 1, 8, 16, 9, 8, ws, ws.numel())
    assert e.value.status == lib.ERR_UNSUPPORTED
    with pytest.raises(DlwpError, match="workspace"):
        lib.launch("dlwp_sph_power_sums_f32", x.device, x, x, tab.wleg, tab.tw, sums, 1, 1, 1, 8, 16, 8, 8, ws, 8)


@pytest.mark.parametrize("grid,nlat,nlon,lmax", [(CE, 32, 64, 16), (LG, 16, 32, 16)])
def test_class_scores_equal_finalize_of_the_reference_sums(grid, nlat, nlon, lmax):
    out, tar = _pair((3, 2, 2, nlat, nlon), 25)
    tar = (0.8 * out + 0.6 * tar).astype(np.float32)                     # coherent at 0.8
    want, f32 = _references(out, tar, grid, lmax, lmax)
    m = SphericalSpectrumMetrics(grid, nlat, nlon, lmax)
    od, td = _dev(out), _dev(tar)
    _check(f"class sums {grid} {nlat}x{nlon} l{lmax}", m.sums(od, td).cpu().numpy(), want, f32)
    got = m(od, td)
    ref, r32 = SR.finalize(want, 3.0), SR.finalize(f32.astype(np.float64), 3.0)
    assert tuple(got["power_pred"].shape) == (2, 2, lmax) and tuple(got["selr"].shape) == (2, 2)
    for key in ("power_pred", "power_true", "power_error", "coherence", "log_ratio", "selr"):
        g = got[key].cpu().numpy()
        assert got[key].dtype == torch.float64
        scale = np.abs(ref[key]).max() if key.startswith("power") else 1.0       # coherence, log ratio: absolute
        err, e32 = np.abs(g - ref[key]).max() / scale, np.abs(r32[key] - ref[key]).max() / scale
        print(f"class {grid} {nlat}x{nlon} {key}: kernel {err:.3e}, float32 restatement {e32:.3e}")
        assert err <= max(8.0 * e32, 1e-6), key
    # running sums through the class, and the workspace that only grows
    run = torch.zeros(4, 2, 2, lmax, dtype=torch.float64, device=DEV)
    assert m.sums(od[:2], td[:2], into=run) is run
    m.sums(od[2:], td[2:], into=run)
    assert torch.equal(run, m.sums(od, td))
    assert len(m._ws[str(od.device)]) == 1
    with pytest.raises(DlwpError, match="built for"):
        m.sums(od[..., :nlat // 2, :], td[..., :nlat // 2, :])


def test_healpix_rollouts_are_remapped_and_scored_bit_for_bit():
    grid, nlat, nlon = LG, 16, 32
    rng = np.random.default_rng(26)
    out = _dev(rng.standard_normal((3, 2, 1, 12, 8, 8)).astype(np.float32))
    tar = _dev(rng.standard_normal((3, 2, 1, 12, 8, 8)).astype(np.float32))
    lons = 360.0 * np.arange(nlon) / nlon
    lats = S.latitudes_deg(grid, nlat)
    plain = SphericalSpectrumMetrics(grid, nlat, nlon)
    want = plain(ops.healpix_to_latlon(out, lats, lons), ops.healpix_to_latlon(tar, lats, lons))
    one_sample = 8 * 2 * 1 * nlat * nlon                                 # a sample of out and of target, remapped
    for budget in (256 << 20, one_sample):
        m = SphericalSpectrumMetrics(grid, nlat, nlon, lons_deg=lons, max_workspace_bytes=budget)
        got = m(out, tar)
        for key, v in want.items():
            assert torch.equal(got[key], v), (budget, key)
    with pytest.raises(DlwpError, match="lons_deg"):
        plain(out, tar)
