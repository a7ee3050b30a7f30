"""Width-generic SpectralConv2d (csrc/spectral_any.hip) on the GPU: every shape the 32-channel kernels do not take.

  * the committed 4-channel fixture of the REAL reference class (unet.py:19-69): output and gradients;
  * the CPU restatement oracle.restate.fno.spectral_conv2d_ref (pinned to the real class by the fixtures) at Ci != Co,
    wide channels, odd H, more than 16 kept columns, widths that are not multiples of 16 or 64;
  * the explicit-row form (_ex) at neuralop's fftshift rows on an odd grid, forward and adjoint;
  * out-of-domain shapes fail with DLWP_ERR_UNSUPPORTED (status -2).
Tolerance: the project's fp32 bound, rel-L2 <= 1e-5."""
import pytest
import torch

from helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-5


def _module(ci, co, m1, m2, seed):
    from dlwp_benchmark_amd.models import SpectralConv2d

    g = torch.Generator().manual_seed(seed)
    mod = SpectralConv2d(ci, co, m1, m2)
    with torch.no_grad():
        mod.weights1.copy_(torch.randn(mod.weights1.shape, generator=g) / ci)
        mod.weights2.copy_(torch.randn(mod.weights2.shape, generator=g) / ci)
    return mod


def test_c4_fixture_forward_and_gradients():
    from dlwp_benchmark_amd import weights as W
    from dlwp_benchmark_amd.models import SpectralConv2d
    from oracle.make_golden import spectral_conv2d_case, tensor_sha

    tag, (ci, co, h, w, m1, m2, b) = "c4_16x16_m4", (4, 4, 16, 16, 4, 4, 2)
    g = load_golden(f"spectral_conv2d_grad_{tag}")
    x, w1, w2 = spectral_conv2d_case(ci, co, h, w, m1, m2, b, tag)
    r = W.normal(f"golden/spectral/{tag}/r", (b, co, h, w), 1.0)
    assert tensor_sha(x, w1, w2, r) == str(g["sha"])
    mod = SpectralConv2d(ci, co, m1, m2)
    with torch.no_grad():
        mod.weights1.copy_(w1)
        mod.weights2.copy_(w2)
    mod = mod.to(DEV)
    want = torch.from_numpy(load_golden(f"spectral_conv2d_{tag}")["y"])
    with torch.no_grad():
        assert rel_l2(mod.eval()(x.to(DEV)), want) <= TOL          # inference plan (host weights)
    mod.train()
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg)                                                     # training plans (_ex, device weights)
    assert rel_l2(y, want) <= TOL
    (y * r.to(DEV)).sum().backward()
    assert rel_l2(xg.grad, torch.from_numpy(g["gx"])) <= TOL
    assert rel_l2(mod.weights1.grad, torch.from_numpy(g["gw1"])) <= TOL
    assert rel_l2(mod.weights2.grad, torch.from_numpy(g["gw2"])) <= TOL


@pytest.mark.parametrize("ci,co,h,w,m1,m2,b", [
    (24, 40, 32, 64, 8, 6, 3),       # Ci != Co, neither a multiple of 16
    (128, 128, 32, 64, 8, 6, 2),     # wide
    (20, 20, 45, 48, 10, 8, 2),      # odd H
    (32, 32, 64, 64, 12, 20, 2),     # 20 kept columns (> 16): 32 channels on the generic path
    (32, 32, 32, 48, 8, 6, 2),       # 32 channels at W = 48: generic path
    (8, 4, 20, 36, 5, 19, 3),        # W a multiple of 4 only; every column kept (W/2 + 1)
    (1, 1, 7, 4, 3, 3, 1),           # smallest grid
])
def test_matches_restatement(ci, co, h, w, m1, m2, b):
    from oracle.restate.fno import spectral_conv2d_ref

    mod = _module(ci, co, m1, m2, seed=ci * 1000 + co + h + w)
    x = torch.randn(b, ci, h, w, generator=torch.Generator().manual_seed(7))
    want = spectral_conv2d_ref(x, mod.weights1.detach(), mod.weights2.detach())
    got = mod.to(DEV).eval()(x.to(DEV))
    torch.cuda.synchronize()
    assert rel_l2(got, want) <= TOL
    # batch independence and run-to-run bit identity
    assert torch.equal(mod(x[-1:].to(DEV)), got[-1:])
    assert torch.equal(mod(x.to(DEV)), got)


@pytest.mark.parametrize("c,h,w,n_modes", [(24, 45, 48, (13, 12)), (64, 33, 64, (12, 40))])
def test_ex_plan_neuralop_rows_forward_and_adjoint(c, h, w, n_modes):
    """SpectralCore form (training.SpectralOperator): fftshift rows of an odd grid, norm="forward" scales; forward
    against the restatement, backward-data against autograd of the same restatement (double precision)."""
    from dlwp_benchmark_amd import training as T
    from oracle.restate.fno import neuralop_kept_rows, neuralop_spectral_conv

    rows_in, rows_out = neuralop_kept_rows(h, n_modes[0])
    n_cols = min(w // 2 + 1, n_modes[1] // 2 + 1)
    g = torch.Generator().manual_seed(c + h)
    wr = torch.randn(c, c, len(rows_in), n_cols, 2, generator=g) / c
    x = torch.randn(2, c, h, w, generator=g)
    dy = torch.randn(2, c, h, w, generator=g)
    op = T.SpectralOperator(c, h, w, rows_in, rows_out, n_cols, 1.0 / (h * w), 1.0, DEV)
    got = op.forward(x.to(DEV), wr.to(DEV))
    wc = torch.view_as_complex(wr.contiguous())
    assert rel_l2(got, neuralop_spectral_conv(x, wc, None, list(n_modes))) <= TOL
    xd = x.double().requires_grad_(True)
    yd = neuralop_spectral_conv_double(xd, wc.to(torch.cdouble), n_modes)
    (yd * dy.double()).sum().backward()
    gx = op.backward_data(dy.to(DEV), wr.to(DEV))
    assert rel_l2(gx, xd.grad) <= TOL


def neuralop_spectral_conv_double(x, weight, n_modes):
    """neuralop_spectral_conv in double precision (autograd reference of the adjoint)."""
    b, ci, h, w = x.shape
    wf = w // 2 + 1
    xf = torch.fft.fftshift(torch.fft.rfftn(x, norm="forward", dim=(-2, -1)), dim=(-2,))
    out = torch.zeros(b, weight.shape[1], h, wf, dtype=torch.cdouble)
    mh, mw = min(h, n_modes[0]), min(wf, n_modes[1] // 2 + 1)
    start = h - mh
    sl_h = slice(start // 2, -start // 2) if start else slice(0, None)
    out[:, :, sl_h, :mw] = torch.einsum("bixy,ioxy->boxy", xf[:, :, sl_h, :mw], weight[:, :, :, :mw])
    return torch.fft.irfftn(torch.fft.fftshift(out, dim=(-2,)), s=(h, w), dim=(-2, -1), norm="forward")


@pytest.mark.parametrize("ci,co,h,w", [(4, 4, 16, 50), (513, 4, 16, 16), (4, 513, 16, 16)])
def test_out_of_domain_is_unsupported(ci, co, h, w):
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.models import SpectralConv2d

    mod = SpectralConv2d(ci, co, 2, 2).to(DEV).eval()
    with pytest.raises(DlwpError, match="status -2"):
        mod(torch.zeros(1, ci, h, w, device=DEV))
