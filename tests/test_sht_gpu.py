"""ops.sht / ops.isht / ops.sph_mix (csrc/sht.hip) against the float64 restatement of tests/sht_ref.py.

Tolerance rule: per case the rel-L2 error of a float32 numpy restatement (the SAME fp32 tables as the device, fp32
accumulation) against float64 is computed; the kernel is allowed 8 x that error -- its summation order differs -- with a floor
of 1e-6 so that tiny cases are not gated by noise.  Every figure is printed before it is asserted; the measured ones stand in
DESIGN.md section 35.  The float64 tables are the independent ones of sht_ref (derivative route) up to lmax 33; above, where
that route is inaccurate, they are sphere.py's float64 tables.
"""
import numpy as np
import pytest
import torch

import sht_ref as R
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd import sphere as S
from dlwp_benchmark_amd.lib import DlwpError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LG, EQ = "legendre-gauss", "equiangular"


def _rel(a, b) -> float:
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def _tables64(grid, nlat, lmax, mmax):
    if max(lmax, mmax) <= R.MAX_INDEPENDENT_L:
        return R.tables(grid, nlat, lmax, mmax)
    theta, w = S.quadrature(grid, nlat)
    return S.legendre(mmax, lmax, theta), w


def _triangular(rng, lead, lmax, mmax):
    c = rng.standard_normal(lead + (lmax, mmax)) + 1j * rng.standard_normal(lead + (lmax, mmax))
    return c * np.tril(np.ones((lmax, mmax)))


# (grid, nlat, nlon, lmax, mmax, leading shape).  The cases: a nlon that is no power of two, lmax != mmax, odd nlat,
# plane counts that are no multiple of the four planes a workgroup takes, the config's grid on both quadratures, and 64 x 128,
# where the m tiles and row chunks of both kernels are more than one.  Two more for paths those do not reach: the Nyquist
# column (mmax = nlon / 2 + 1, whose imaginary part the inverse drops) and the corner of the envelope (256 x 512, every tile
# extent cut down to fit the LDS budget).
CASES = [(LG, 8, 16, 8, 8, (1,)), (LG, 8, 16, 8, 8, (15,)), (LG, 12, 20, 7, 5, (7,)), (EQ, 9, 16, 4, 4, (3,)),
         (EQ, 32, 64, 32, 32, (3, 5)), (LG, 32, 64, 32, 32, (64,)), (LG, 64, 128, 64, 64, (4,)), (LG, 12, 16, 10, 9, (2,)),
         (LG, 256, 512, 256, 257, (2,))]
IDS = [f"{g[:2]}-{a}x{b}-l{l}-m{m}-p{'x'.join(map(str, p))}" for g, a, b, l, m, p in CASES]


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax,lead", CASES, ids=IDS)
def test_sht_against_float64(grid, nlat, nlon, lmax, mmax, lead):
    rng = np.random.default_rng(11)
    x = rng.standard_normal(lead + (nlat, nlon)).astype(np.float32)
    p, w = _tables64(grid, nlat, lmax, mmax)
    want = R.sht(x.astype(np.float64), p, w).numpy()
    wleg32, _ = S.tables_f32(grid, nlat, lmax, mmax)
    e32 = _rel(R.sht_f32(x, wleg32, S.twiddles(nlon).astype(np.float32)), want)
    xd = torch.from_numpy(x).to(DEV)
    got = ops.sht(xd, grid, lmax, mmax)
    again = ops.sht(xd, grid, lmax, mmax)
    assert got.dtype == torch.complex64 and tuple(got.shape) == lead + (lmax, mmax)
    err = _rel(got.cpu().numpy(), want)
    print(f"sht {grid} {nlat}x{nlon} l{lmax} m{mmax} {lead}: kernel {err:.3e}, float32 restatement {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(again))
    upper = np.triu(np.ones((lmax, mmax), dtype=bool), 1)
    g = got.cpu().numpy()
    assert np.all(g[..., upper] == 0)


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax,lead", CASES, ids=IDS)
def test_isht_against_float64(grid, nlat, nlon, lmax, mmax, lead):
    rng = np.random.default_rng(12)
    c = _triangular(rng, lead, lmax, mmax).astype(np.complex64)
    p, _ = _tables64(grid, nlat, lmax, mmax)
    want = R.isht(c.astype(np.complex128), p, nlon).numpy()
    _, leg32 = S.tables_f32(grid, nlat, lmax, mmax)
    e32 = _rel(R.isht_f32(c, leg32, S.twiddles(nlon).astype(np.float32), nlon), want)
    poisoned = c.copy()                                   # the l < m triangle is never read: NaN there changes nothing
    poisoned[..., np.triu(np.ones((lmax, mmax), dtype=bool), 1)] = np.nan
    cd = torch.from_numpy(poisoned).to(DEV)
    got = ops.isht(cd, grid, nlat, nlon)
    again = ops.isht(cd, grid, nlat, nlon)
    assert got.dtype == torch.float32 and tuple(got.shape) == lead + (nlat, nlon)
    err = _rel(got.cpu().numpy(), want)
    print(f"isht {grid} {nlat}x{nlon} l{lmax} m{mmax} {lead}: kernel {err:.3e}, float32 restatement {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)
    assert torch.equal(got, again)


def test_round_trip_on_the_device():
    grid, nlat, nlon, lmax = LG, 32, 64, 32
    rng = np.random.default_rng(13)
    c = _triangular(rng, (6,), lmax, lmax)
    c[..., 0] = c[..., 0].real
    p, _ = R.tables(grid, nlat, lmax, lmax)
    x64 = R.isht(c, p, nlon).numpy()                      # band limited: the round trip is exact in exact arithmetic
    x = x64.astype(np.float32)
    wleg32, leg32 = S.tables_f32(grid, nlat, lmax, lmax)
    tw32 = S.twiddles(nlon).astype(np.float32)
    e32 = _rel(R.isht_f32(R.sht_f32(x, wleg32, tw32), leg32, tw32, nlon), x64)
    got = ops.isht(ops.sht(torch.from_numpy(x).to(DEV), grid, lmax, lmax), grid, nlat, nlon)
    err = _rel(got.cpu().numpy(), x64)
    print(f"device round trip lg 32x64 l32: kernel {err:.3e}, float32 restatement {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)


# (B, Ci, Co, lmax, mmax): four (one 16-row tile; exact tiles; K and N tails with several row blocks; the config's
# widths, eight K stages and four output tiles) and one with mmax < lmax (rows per degree stop growing at mmax)
MIX = [(1, 3, 5, 4, 4), (2, 16, 16, 8, 8), (3, 40, 24, 32, 32), (2, 256, 256, 32, 32), (2, 5, 70, 9, 6)]


@pytest.mark.parametrize("b,ci,co,lmax,mmax", MIX, ids=[f"b{b}-i{i}-o{o}-l{l}-m{m}" for b, i, o, l, m in MIX])
def test_sph_mix_against_float64(b, ci, co, lmax, mmax):
    rng = np.random.default_rng(14)
    c = _triangular(rng, (b, ci), lmax, mmax).astype(np.complex64)
    wt = ((rng.standard_normal((ci, co, lmax)) + 1j * rng.standard_normal((ci, co, lmax))) / np.sqrt(ci)).astype(np.complex64)
    want = R.sph_mix(c.astype(np.complex128), wt.astype(np.complex128)).numpy()
    e32 = _rel(R.sph_mix_f32(c, wt), want)
    upper = np.triu(np.ones((lmax, mmax), dtype=bool), 1)
    poisoned = c.copy()
    poisoned[..., upper] = np.nan                         # proves the triangle above the diagonal is not read
    cd, wd = torch.from_numpy(poisoned).to(DEV), torch.from_numpy(wt).to(DEV)
    got = ops.sph_mix(cd, wd)
    again = ops.sph_mix(cd, wd)
    g = got.cpu().numpy()
    err = _rel(g, want)
    print(f"sph_mix b{b} ci{ci} co{co} l{lmax} m{mmax}: kernel {err:.3e}, float32 restatement {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)
    assert np.all(g[..., upper] == 0)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(again))
    # the cached degree-major pack (owner given): the same sums in the same order, and re-made when the owner is written to
    owner = torch.view_as_real(wd)
    packed = ops.sph_mix(cd, wd, owner=owner)
    assert torch.equal(torch.view_as_real(packed), torch.view_as_real(got))
    owner.mul_(2.0)
    doubled = ops.sph_mix(cd, wd, owner=owner)
    assert torch.equal(torch.view_as_real(doubled), 2.0 * torch.view_as_real(got))


def test_autograd_against_float64():
    """gradients of a scalar loss through the three ops (HIP forward, torch-form backward) against autograd of the float64
    restatement: the project's training bound, 1e-6 relative"""
    grid, nlat, nlon, lmax = LG, 8, 16, 8
    rng = np.random.default_rng(15)
    p, w = R.tables(grid, nlat, lmax, lmax)
    x = rng.standard_normal((2, 3, nlat, nlon)).astype(np.float32)
    gc = _triangular(rng, (2, 3), lmax, lmax).astype(np.complex64)
    gx = rng.standard_normal((2, 3, nlat, nlon)).astype(np.float32)
    c = _triangular(rng, (2, 3), lmax, lmax).astype(np.complex64)
    wt = ((rng.standard_normal((3, 3, lmax)) + 1j * rng.standard_normal((3, 3, lmax))) / np.sqrt(3)).astype(np.complex64)

    def loss_c(out, g):            # a real scalar of a complex output
        return (out * g.conj()).real.sum()

    def both(fn_dev, fn_ref, inputs, cotangent, complex_out):
        dev = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in inputs]
        ref = [torch.from_numpy(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)).requires_grad_(True) for a in inputs]
        gd, gr = torch.from_numpy(cotangent).to(DEV), torch.from_numpy(cotangent)
        od, orf = fn_dev(*dev), fn_ref(*ref)
        assert od.requires_grad
        (loss_c(od, gd) if complex_out else (od * gd).sum()).backward()
        (loss_c(orf, gr.to(torch.complex128)) if complex_out else (orf * gr.double()).sum()).backward()
        return [(d.grad.cpu().numpy(), r.grad.numpy()) for d, r in zip(dev, ref)]

    for name, pairs in (
            ("sht", both(lambda t: ops.sht(t, grid, lmax, lmax), lambda t: R.sht(t, p, w), [x], gc, True)),
            ("isht", both(lambda t: ops.isht(t, grid, nlat, nlon), lambda t: R.isht(t, p, nlon), [c], gx, False)),
            ("sph_mix", both(ops.sph_mix, R.sph_mix, [c, wt], gc, True))):
        for i, (got, want) in enumerate(pairs):
            err = _rel(got, want)
            print(f"grad {name} input {i}: {err:.3e}")
            assert err <= 1e-6


def test_arguments_are_checked():
    x = torch.zeros(2, 8, 16, device=DEV)
    with pytest.raises(DlwpError):
        ops.sht(torch.zeros(2, 8, 16), LG)                               # a CPU tensor
    with pytest.raises(DlwpError):
        ops.sht(torch.zeros(2, 8, 15, device=DEV), LG)                   # odd nlon
    with pytest.raises(DlwpError):
        ops.sht(x, LG, 9, 8)                                             # lmax > nlat
    with pytest.raises(DlwpError):
        ops.isht(torch.zeros(2, 8, 8, device=DEV), LG, 8, 16)            # real coefficients
    with pytest.raises(NotImplementedError):
        ops.sht(x, "lobatto")
    with pytest.raises(DlwpError):
        ops.sph_mix(torch.zeros(1, 3, 4, 4, dtype=torch.complex64, device=DEV), torch.zeros(2, 3, 4, dtype=torch.complex64, device=DEV))
