"""ops.sht_backward / ops.isht_backward / ops.sph_mix_backward (csrc/sht.hip) and the autograd Functions on top of them, against
float64 autograd of tests/sht_ref.py (tests/sht_bwd_ref.py).

Tolerance rule (as tests/test_sht_gpu.py): per case the rel-L2 error of the float32 numpy restatement
(the SAME fp32 tables as the device, fp32 accumulation) against float64 is computed; the kernel is allowed 8 x that error -- its
summation order differs -- with a floor of 1e-6.  Every figure is printed before it is asserted; the measured ones stand in
DESIGN.md section 35.7.  Float64 tables: the independent ones of sht_ref up to lmax 33, sphere.py's above.
"""
import numpy as np
import pytest
import torch

import sht_bwd_ref as B
import sht_ref as R
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd import sphere as S
from dlwp_benchmark_amd import training as T
from dlwp_benchmark_amd.lib import DlwpError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LG, EQ = "legendre-gauss", "equiangular"


def _tables64(grid, nlat, lmax, mmax):
    if max(lmax, mmax) <= R.MAX_INDEPENDENT_L:
        return R.tables(grid, nlat, lmax, mmax)
    theta, w = S.quadrature(grid, nlat)
    return S.legendre(mmax, lmax, theta), w


def _bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _random_complex(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


# (grid, nlat, nlon, lmax, mmax, leading shape): the forward's cases for the forward's reasons -- a nlon that is no power of two,
# lmax != mmax, odd nlat, plane counts that are no multiple of the four planes a workgroup takes, the Nyquist column, several m
# tiles and row chunks (64 x 128), and the corner of the envelope, where every tile extent is cut down to fit LDS.
CASES = [(LG, 8, 16, 8, 8, (1,)), (LG, 8, 16, 8, 8, (15,)), (LG, 12, 20, 7, 5, (7,)), (EQ, 9, 16, 4, 4, (3,)),
         (LG, 12, 16, 10, 9, (2,)), (LG, 32, 64, 32, 32, (6,)), (LG, 64, 128, 64, 64, (4,)), (LG, 256, 512, 256, 257, (2,))]
IDS = [f"{g[:2]}-{a}x{b}-l{l}-m{m}-p{'x'.join(map(str, p))}" for g, a, b, l, m, p in CASES]


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax,lead", CASES, ids=IDS)
def test_sht_backward_against_float64(grid, nlat, nlon, lmax, mmax, lead):
    rng = np.random.default_rng(31)
    g = _random_complex(rng, lead + (lmax, mmax))
    p, w = _tables64(grid, nlat, lmax, mmax)
    want = B.truth_sht_bwd(g, p, w, nlat, nlon)
    wleg32, _ = S.tables_f32(grid, nlat, lmax, mmax)
    e32 = B.rel(B.sht_bwd_f32(g, wleg32, S.twiddles(nlon).astype(np.float32), nlon), want)
    gd = torch.from_numpy(g).to(DEV)
    got = ops.sht_backward(gd, grid, nlat, nlon)
    again = ops.sht_backward(gd, grid, nlat, nlon)
    assert got.dtype == torch.float32 and tuple(got.shape) == lead + (nlat, nlon)
    err = B.rel(got.cpu().numpy(), want)
    print(f"sht_backward {grid} {nlat}x{nlon} l{lmax} m{mmax} {lead}: kernel {err:.3e}, float32 restatement {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)
    assert torch.equal(got, again)
    poisoned = g.copy()                                   # the l < m triangle of the cotangent is never read
    poisoned[..., np.triu(np.ones((lmax, mmax), dtype=bool), 1)] = np.nan
    assert torch.equal(ops.sht_backward(torch.from_numpy(poisoned).to(DEV), grid, nlat, nlon), got)


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax,lead", CASES, ids=IDS)
def test_isht_backward_against_float64(grid, nlat, nlon, lmax, mmax, lead):
    rng = np.random.default_rng(32)
    gy = rng.standard_normal(lead + (nlat, nlon)).astype(np.float32)
    p, _ = _tables64(grid, nlat, lmax, mmax)
    want = B.truth_isht_bwd(gy, p, lmax, mmax)
    _, leg32 = S.tables_f32(grid, nlat, lmax, mmax)
    e32 = B.rel(B.isht_bwd_f32(gy, leg32, S.twiddles(nlon).astype(np.float32)), want)
    gd = torch.from_numpy(gy).to(DEV)
    got = ops.isht_backward(gd, grid, lmax, mmax)
    again = ops.isht_backward(gd, grid, lmax, mmax)
    assert got.dtype == torch.complex64 and tuple(got.shape) == lead + (lmax, mmax)
    gn = got.cpu().numpy()
    err = B.rel(gn, want)
    print(f"isht_backward {grid} {nlat}x{nlon} l{lmax} m{mmax} {lead}: kernel {err:.3e}, float32 restatement {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)
    assert torch.equal(_bits(got), _bits(again))
    assert np.all(gn[..., np.triu(np.ones((lmax, mmax), dtype=bool), 1)] == 0)


def _identity_error(lhs: float, rhs: float) -> float:
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs))


@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax", [(LG, 32, 64, 32, 32), (LG, 12, 16, 10, 9)], ids=["lg-32x64-l32", "lg-12x16-l10-m9"])
def test_dot_product_identities_on_the_device(grid, nlat, nlon, lmax, mmax):
    """<sht x, g> = <x, sht_backward g> and <isht c, gy> = <c, isht_backward gy>, both sides summed in float64 on the host.  The
    cotangents are the operator's own output plus noise, so neither side is a small difference of large terms.  Bound: 8 x the
    error of the same identity evaluated with the float32 restatements, floor 1e-6."""
    rng = np.random.default_rng(33)
    wleg32, leg32 = S.tables_f32(grid, nlat, lmax, mmax)
    tw32 = S.twiddles(nlon).astype(np.float32)
    x = rng.standard_normal((5, nlat, nlon)).astype(np.float32)
    c = B.triangular(rng, (5,), lmax, mmax).astype(np.complex64)
    g = (R.sht_f32(x, wleg32, tw32) + 0.5 * B.triangular(rng, (5,), lmax, mmax)).astype(np.complex64)
    gy = (R.isht_f32(c, leg32, tw32, nlon) + 0.5 * rng.standard_normal((5, nlat, nlon))).astype(np.float32)
    xd, cd, gd, gyd = (torch.from_numpy(a).to(DEV) for a in (x, c, g, gy))

    e32 = _identity_error(B.dot64(R.sht_f32(x, wleg32, tw32), g), B.dot64(x, B.sht_bwd_f32(g, wleg32, tw32, nlon)))
    lhs = B.dot64(ops.sht(xd, grid, lmax, mmax).cpu().numpy(), g)
    rhs = B.dot64(x, ops.sht_backward(gd, grid, nlat, nlon).cpu().numpy())
    err = _identity_error(lhs, rhs)
    print(f"<sht x, g> = <x, sht_backward g> {nlat}x{nlon} l{lmax} m{mmax}: device {err:.3e} ({lhs:.9e} / {rhs:.9e}), float32 {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)

    e32 = _identity_error(B.dot64(R.isht_f32(c, leg32, tw32, nlon), gy), B.dot64(c, B.isht_bwd_f32(gy, leg32, tw32)))
    lhs = B.dot64(ops.isht(cd, grid, nlat, nlon).cpu().numpy(), gy)
    rhs = B.dot64(c, ops.isht_backward(gyd, grid, lmax, mmax).cpu().numpy())
    err = _identity_error(lhs, rhs)
    print(f"<isht c, gy> = <c, isht_backward gy> {nlat}x{nlon} l{lmax} m{mmax}: device {err:.3e} ({lhs:.9e} / {rhs:.9e}), float32 {e32:.3e}")
    assert err <= max(8.0 * e32, 1e-6)


# (B, Ci, Co, lmax, mmax): the forward's five -- (1, 3, 5, 4, 4) has K = 1 at degree 0 and every tail of the weight-gradient kernel
# (M, N and K), (2, 256, 256, 32, 32) the config's widths: sixteen (i, o) tiles -- and (16, 8, 8, 32, 32), K = 512: the longest K
# chain, sixteen chunks
MIX = [(1, 3, 5, 4, 4), (2, 16, 16, 8, 8), (3, 40, 24, 32, 32), (2, 256, 256, 32, 32), (2, 5, 70, 9, 6), (16, 8, 8, 32, 32)]


@pytest.mark.parametrize("b,ci,co,lmax,mmax", MIX, ids=[f"b{b}-i{i}-o{o}-l{l}-m{m}" for b, i, o, l, m in MIX])
def test_sph_mix_backward_against_float64(b, ci, co, lmax, mmax):
    rng = np.random.default_rng(34)
    upper = np.triu(np.ones((lmax, mmax), dtype=bool), 1)
    c = _random_complex(rng, (b, ci, lmax, mmax))
    g = _random_complex(rng, (b, co, lmax, mmax))
    wt = (_random_complex(rng, (ci, co, lmax)) / np.sqrt(ci)).astype(np.complex64)
    want_c, want_w = B.truth_sph_mix_bwd(c, wt, g)
    e32c, e32w = B.rel(B.sph_mix_dgrad_f32(g, wt), want_c), B.rel(B.sph_mix_wgrad_f32(c, g), want_w)
    cd, wd, gd = (torch.from_numpy(a).to(DEV) for a in (c, wt, g))
    gc, gw = ops.sph_mix_backward(cd, wd, gd)
    assert gc.dtype == gw.dtype == torch.complex64
    assert tuple(gc.shape) == (b, ci, lmax, mmax) and tuple(gw.shape) == (ci, co, lmax)
    errc, errw = B.rel(gc.cpu().numpy(), want_c), B.rel(gw.cpu().numpy(), want_w)
    print(f"sph_mix_backward b{b} ci{ci} co{co} l{lmax} m{mmax}: gc_in kernel {errc:.3e}, float32 restatement {e32c:.3e}; "
          f"gw kernel {errw:.3e}, float32 restatement {e32w:.3e}")
    assert errc <= max(8.0 * e32c, 1e-6)
    assert errw <= max(8.0 * e32w, 1e-6)
    assert np.all(gc.cpu().numpy()[..., upper] == 0)
    gc2, gw2 = ops.sph_mix_backward(cd, wd, gd)
    assert torch.equal(_bits(gc), _bits(gc2)) and torch.equal(_bits(gw), _bits(gw2))
    # neither operand is read above the diagonal
    cp, gp = c.copy(), g.copy()
    cp[..., upper] = np.nan
    gp[..., upper] = np.nan
    gc3, gw3 = ops.sph_mix_backward(torch.from_numpy(cp).to(DEV), wd, torch.from_numpy(gp).to(DEV))
    assert torch.equal(_bits(gc), _bits(gc3)) and torch.equal(_bits(gw), _bits(gw3))
    # one half only
    only_w = ops.sph_mix_backward(cd, wd, gd, need_c=False)
    only_c = ops.sph_mix_backward(cd, wd, gd, need_w=False)
    assert only_w[0] is None and torch.equal(_bits(only_w[1]), _bits(gw))
    assert only_c[1] is None and torch.equal(_bits(only_c[0]), _bits(gc))
    # the two candidates of each half sum in the same order
    for dgrad, wgrad in (("in_place", "direct"), ("packed", "packed")):
        gc4, gw4 = ops.sph_mix_backward(cd, wd, gd, dgrad=dgrad, wgrad=wgrad)
        assert torch.equal(_bits(gc), _bits(gc4)) and torch.equal(_bits(gw), _bits(gw4))


def _three_op_gradients():
    """gradients of a scalar through ops.sht -> ops.sph_mix -> ops.isht and through each op alone, at lg 8 x 16 l8, 2 x 3 channels"""
    grid, nlat, nlon, lmax = LG, 8, 16, 8
    rng = np.random.default_rng(35)
    x = torch.from_numpy(rng.standard_normal((2, 3, nlat, nlon)).astype(np.float32)).to(DEV).requires_grad_(True)
    c = torch.from_numpy(B.triangular(rng, (2, 3), lmax, lmax).astype(np.complex64)).to(DEV).requires_grad_(True)
    wt = torch.from_numpy((_random_complex(rng, (3, 3, lmax)) / np.sqrt(3)).astype(np.complex64)).to(DEV).requires_grad_(True)
    gy = torch.from_numpy(rng.standard_normal((2, 3, nlat, nlon)).astype(np.float32)).to(DEV)
    gc = torch.from_numpy(_random_complex(rng, (2, 3, lmax, lmax))).to(DEV)
    chain = ops.isht(ops.sph_mix(ops.sht(x, grid, lmax, lmax), wt), grid, nlat, nlon)
    alone = ops.isht(c, grid, nlat, nlon)
    mixed = ops.sph_mix(c, wt)
    assert chain.requires_grad and alone.requires_grad and mixed.requires_grad
    loss = (chain * gy).sum() + (alone * gy).sum() + (mixed * gc.conj()).real.sum()
    return torch.autograd.grad(loss, (x, c, wt))


def test_functions_take_the_hip_backward(monkeypatch):
    """fails on a tree whose Functions differentiate the torch forms"""
    from dlwp_benchmark_amd.models import SFNO2DModule
    from dlwp_benchmark_amd.weights import fill_state_dict

    def refuse(*a, **k):
        raise AssertionError("the torch form was differentiated on the default path")

    monkeypatch.delenv("DLWP_TRAIN_TORCH_BACKWARD", raising=False)
    monkeypatch.setattr(T, "_grad_of_torch_form", refuse)
    for g in _three_op_gradients():
        assert bool(torch.isfinite(_bits(g)).all())
    model = SFNO2DModule(constant_channels=2, prescribed_channels=1, prognostic_channels=3, height=8, width=16, grid=LG,
                         num_layers=2, scale_factor=1, context_size=1, use_mlp=True, big_skip=True, pos_embed=True, embed_dim=16)
    fill_state_dict(model, std_fn=lambda n, s: 0.7 / s[0] ** 0.5 if n.endswith("filter.filter.weight") else None)
    model = model.to(DEV).train()
    gen = torch.Generator().manual_seed(3)
    const, presc, prog = torch.randn(2, 1, 2, 8, 16, generator=gen), torch.randn(2, 3, 1, 8, 16, generator=gen), torch.randn(2, 3, 3, 8, 16, generator=gen)
    out = model(constants=const.to(DEV), prescribed=presc.to(DEV), prognostic=prog.to(DEV))
    assert out.requires_grad
    out.square().sum().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(model.sfno.blocks[0].filter.filter.weight.grad.abs().max()) > 0


def test_torch_backward_switch_reaches_the_torch_forms_and_agrees(monkeypatch):
    monkeypatch.delenv("DLWP_TRAIN_TORCH_BACKWARD", raising=False)
    hip = _three_op_gradients()
    calls = []
    inner = T._grad_of_torch_form

    def counting(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    monkeypatch.setattr(T, "_grad_of_torch_form", counting)
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    ref = _three_op_gradients()
    assert len(calls) == 5, len(calls)                    # sht, the two isht, the two sph_mix
    for name, a, b in zip(("x", "c", "weight"), hip, ref):
        err = B.rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"HIP backward against the torch form, grad {name}: {err:.3e}")
        assert err <= 1e-6


def test_arguments_are_checked():
    c = torch.zeros(2, 8, 8, dtype=torch.complex64, device=DEV)
    with pytest.raises(DlwpError):
        ops.sht_backward(torch.zeros(2, 8, 8, dtype=torch.complex64), LG, 8, 16)             # CPU tensors
    with pytest.raises(DlwpError):
        ops.isht_backward(torch.zeros(2, 8, 16), LG, 8, 8)
    with pytest.raises(DlwpError):
        ops.sph_mix_backward(torch.zeros(1, 3, 4, 4, dtype=torch.complex64), torch.zeros(3, 5, 4, dtype=torch.complex64),
                             torch.zeros(1, 5, 4, 4, dtype=torch.complex64))
    with pytest.raises(DlwpError):
        ops.sht_backward(torch.zeros(2, 8, 8, device=DEV), LG, 8, 16)                        # a real cotangent
    with pytest.raises(DlwpError):                                                           # g has cin channels, not cout
        ops.sph_mix_backward(torch.zeros(1, 3, 4, 4, dtype=torch.complex64, device=DEV),
                             torch.zeros(3, 5, 4, dtype=torch.complex64, device=DEV),
                             torch.zeros(1, 3, 4, 4, dtype=torch.complex64, device=DEV))
    with pytest.raises(DlwpError):
        ops.sht_backward(torch.zeros(2, 9, 8, dtype=torch.complex64, device=DEV), LG, 8, 16)  # lmax > nlat
    with pytest.raises(DlwpError):
        ops.isht_backward(torch.zeros(2, 8, 16, device=DEV), LG, 9, 8)
    with pytest.raises(NotImplementedError):
        ops.sht_backward(c, "lobatto", 8, 16)
    with pytest.raises(NotImplementedError):
        ops.isht_backward(torch.zeros(2, 8, 16, device=DEV), "lobatto", 8, 8)
