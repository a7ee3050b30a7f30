"""The HEALPix backward kernels (csrc/healpix_bwd.hip) on the GPU.

  dlwp_conv3x3_hpx_bwd_data_f32  dX of HEALPixPadding(1) + Conv2d(3x3) against fp64 autograd of training.conv3x3_torch with
                                 the HEALPix table, rel-L2 <= 1e-5, over nside x Cin x Cout; through the autograd function
                                 with two input segments, every pre- / post-activation and a residual
  dlwp_healpix_pad_bwd_f32       the adjoint of the padding at p in {1, 2, nside} against fp64 autograd and against the
                                 gradients of the REAL HEALPixPadding (tests/golden/healpix_pad_grad_p*.npz)
plus bitwise reruns, batch independence and the rejection of bad shapes and pointers."""
import os
import sys

import pytest
import torch

from helpers import load_golden, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CHANNELS = [1, 3, 17, 64, 136]


def _randn(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).to(DEV)


def _table(n, p=1):
    from dlwp_benchmark_amd import healpix as H

    return H.pad_table(n, n, p).to(DEV)


def _fp64_conv_grads(x0, x1, w, b, resid, pre_act, act, gy):
    """fp64 autograd of the torch restatement: gradients of every tensor argument"""
    from dlwp_benchmark_amd import training as T

    ins = [t.detach().double().requires_grad_(True) if t is not None else None for t in (x0, x1, w, b, resid)]
    y = T.conv3x3_torch(ins[0], ins[1], ins[2], ins[3], ins[4], pre_act, act, _table(x0.shape[2]))
    wrt = [t for t in ins if t is not None]
    return list(torch.autograd.grad(y, wrt, gy.double()))


@pytest.mark.gpu
@pytest.mark.parametrize("nside", [1, 2, 4, 8, 32])
@pytest.mark.parametrize("cin", CHANNELS)
@pytest.mark.parametrize("cout", CHANNELS)
def test_bwd_data_matches_fp64_autograd(nside, cin, cout):
    from dlwp_benchmark_amd import ops

    faces = 12 if nside == 32 else 24
    seed = 1000 * nside + 10 * cin + cout
    x = _randn((faces, cin, nside, nside), seed)
    w = _randn((cout, cin, 3, 3), seed + 1) * (1.0 / (9 * cin) ** 0.5)
    gy = _randn((faces, cout, nside, nside), seed + 2)
    want, _ = _fp64_conv_grads(x, None, w, None, None, 0, 0, gy)
    got = ops.conv3x3_hpx_backward_data(gy, w, cin)
    assert got.shape == x.shape
    assert rel_l2(got, want) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("pre_act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("with_resid", [False, True])
def test_conv_function_gradients_two_segments(pre_act, act, with_resid):
    """training.conv3x3 (hpx=True): dX0, dX1 through the new kernel, dW, db, dresid, every activation pairing"""
    from dlwp_benchmark_amd import training as T

    n, c0, c1, cout, faces = 8, 5, 3, 7, 24
    seed = 100 * pre_act + 10 * act + int(with_resid)
    x0, x1 = _randn((faces, c0, n, n), seed), _randn((faces, c1, n, n), seed + 1)
    w = _randn((cout, c0 + c1, 3, 3), seed + 2) * 0.3
    b = _randn((cout,), seed + 3)
    resid = _randn((faces, cout, n, n), seed + 4) if with_resid else None
    gy = _randn((faces, cout, n, n), seed + 5)
    want = _fp64_conv_grads(x0, x1, w, b, resid, pre_act, act, gy)
    ins = [t.clone().requires_grad_(True) if t is not None else None for t in (x0, x1, w, b, resid)]
    y = T.conv3x3(ins[0], ins[2], ins[3], act=act, x1=ins[1], pre_act=pre_act, resid=ins[4], hpx=True)
    y.backward(gy)
    got = [t.grad for t in ins if t is not None]
    for name, g, r in zip(("x0", "x1", "weight", "bias", "resid"), got, want):
        assert rel_l2(g, r) <= 1e-5, name


@pytest.mark.gpu
@pytest.mark.parametrize("nside", [4, 32])
@pytest.mark.parametrize("cout", [17, 64, 136])
def test_conv_function_input_gradient_both_forms(nside, cout):
    """the direct kernel up to HPX_DX_DIRECT_MAX_COUT output channels, the two-step form above: same gradient"""
    from dlwp_benchmark_amd import training as T

    cin, faces = 24, 12
    x = _randn((faces, cin, nside, nside), 3 * cout + nside).requires_grad_(True)
    w = _randn((cout, cin, 3, 3), cout) * (1.0 / (9 * cin) ** 0.5)
    gy = _randn((faces, cout, nside, nside), cout + 1)
    want, _ = _fp64_conv_grads(x, None, w, None, None, 0, 0, gy)
    T.conv3x3(x, w.requires_grad_(True), None, hpx=True).backward(gy)
    assert rel_l2(x.grad, want) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("nside,p", sorted({(n, p) for n in (1, 2, 4, 8) for p in (1, 2, n) if p <= n}))
def test_pad_backward_matches_fp64_autograd(nside, p):
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd import training as T

    x = _randn((24, 3, nside, nside), 7 * nside + p, torch.float64).requires_grad_(True)
    gy = _randn((24, 3, nside + 2 * p, nside + 2 * p), 11 * nside + p)
    want, = torch.autograd.grad(T._hpx_pad_torch(x, _table(nside, p)), x, gy.double())
    got = ops.healpix_pad_backward(gy, p)
    assert got.shape == x.shape
    assert rel_l2(got, want) <= 1e-6


def _pad_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_hpx_grad as tool
    finally:
        sys.path.pop(0)
    return tool


@pytest.mark.gpu
@pytest.mark.parametrize("p", [1, 2, 4])
def test_differentiable_padding_matches_reference_golden(p):
    """models.HEALPixPadding(p) with autograd against the REAL class's dL/dx for sum(pad(x) * r)"""
    from dlwp_benchmark_amd import weights as W
    from dlwp_benchmark_amd.models.unet import HEALPixPadding

    tool = _pad_tool()
    g = load_golden(f"healpix_pad_grad_p{p}")
    b, c, n = tool.PAD_CASES[p]
    xn, rn = tool.pad_names(p)
    x = W.normal(xn, (b * 12, c, n, n), 1.0).to(DEV).requires_grad_(True)
    r = W.normal(rn, (b * 12, c, n + 2 * p, n + 2 * p), 1.0).to(DEV)
    loss = (HEALPixPadding(padding=p)(x) * r).sum()
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    assert rel_l2(x.grad, torch.from_numpy(g["grad_x"])) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("p", [2, 3])
def test_padding_beyond_one_is_differentiable(p):
    """HEALPixPadding(2) and (3) used to raise 'differentiable HEALPix padding is built for padding 1'"""
    from dlwp_benchmark_amd import training as T
    from dlwp_benchmark_amd.models.unet import HEALPixPadding

    x = _randn((24, 4, 8, 8), 50 + p).requires_grad_(True)
    y = HEALPixPadding(padding=p)(x)
    assert y.shape == (24, 4, 8 + 2 * p, 8 + 2 * p) and y.requires_grad
    gy = _randn(tuple(y.shape), 60 + p)
    y.backward(gy)
    x64 = x.detach().double().requires_grad_(True)
    want, = torch.autograd.grad(T._hpx_pad_torch(x64, _table(8, p)), x64, gy.double())
    assert torch.equal(y.detach(), T._hpx_pad_torch(x.detach(), _table(8, p)))
    assert rel_l2(x.grad, want) <= 1e-6


@pytest.mark.gpu
def test_bitwise_reruns_and_batch_independence():
    from dlwp_benchmark_amd import ops

    n, cin, cout = 16, 17, 64
    gy = _randn((36, cout, n, n), 1)
    w = _randn((cout, cin, 3, 3), 2)
    a = ops.conv3x3_hpx_backward_data(gy, w, cin)
    b = ops.conv3x3_hpx_backward_data(gy, w, cin)
    one = ops.conv3x3_hpx_backward_data(gy[12:24].clone(), w, cin)
    assert torch.equal(a, b)
    assert torch.equal(a[12:24], one)
    dy = _randn((36, 5, n + 4, n + 4), 3)
    pa, pb = ops.healpix_pad_backward(dy, 2), ops.healpix_pad_backward(dy, 2)
    assert torch.equal(pa, pb)
    assert torch.equal(pa[24:36], ops.healpix_pad_backward(dy[24:36].clone(), 2))


@pytest.mark.gpu
def test_bad_shapes_and_pointers_are_rejected():
    from dlwp_benchmark_amd import healpix as H
    from dlwp_benchmark_amd import lib, ops

    gy = _randn((24, 4, 8, 8), 9)
    w = _randn((4, 3, 3, 3), 10)
    with pytest.raises(lib.DlwpError):
        ops.conv3x3_hpx_backward_data(gy[:23], w, 3)                        # not (batch * 12) faces
    with pytest.raises(lib.DlwpError):
        ops.conv3x3_hpx_backward_data(gy, w, 5)                             # weight does not match cin
    with pytest.raises(lib.DlwpError):
        ops.conv3x3_hpx_backward_data(gy.cpu(), w, 3)
    with pytest.raises(lib.DlwpError):
        ops.healpix_pad_backward(_randn((24, 2, 10, 12), 11), 1)            # not a square face
    with pytest.raises(lib.DlwpError):
        ops.healpix_pad_backward(_randn((20, 2, 10, 10), 12), 1)

    L = lib.load()
    adj = H.device_adjoint_table(8, 8, 1, DEV)
    dx = torch.empty(24, 3, 8, 8, device=DEV)
    ptrs = (adj.indptr.data_ptr(), adj.index.data_ptr(), adj.weight.data_ptr())
    nbytes = L.dlwp_conv3x3_hpx_bwd_data_workspace_bytes(24, 8, 8, 3)
    assert nbytes == 24 * 3 * (2 * 10 + 2 * 8) * 4
    ring = torch.empty(nbytes // 4, device=DEV)
    conv = lambda *a: L.dlwp_conv3x3_hpx_bwd_data_f32(*a, None)
    ok = (gy.data_ptr(), w.data_ptr(), dx.data_ptr(), 24, 8, 8, 3, 4) + ptrs + (ring.data_ptr(), nbytes)
    assert conv(*ok) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, ops.conv3x3_hpx_backward_data(gy, w, 3))
    for i in (0, 1, 2, 8, 9, 10, 11):                                           # null pointers
        assert conv(*(ok[:i] + (None,) + ok[i + 1:])) == -1
    assert conv(*(ok[:12] + (nbytes - 4,))) == -4                              # workspace too small
    assert conv(*(ok[:3] + (18,) + ok[4:])) == -1                               # n_faces not a multiple of 12
    assert conv(*(ok[:4] + (8, 9) + ok[6:])) == -1                              # not square
    assert conv(*(ok[:6] + (0,) + ok[7:])) == -1                                # no channels
    assert conv(*(ok[:3] + (65544,) + ok[4:])) == -2                            # beyond the grid
    assert b"65535" in L.dlwp_last_error()
    pad = lambda *a: L.dlwp_healpix_pad_bwd_f32(*a, None)
    dy = _randn((24, 3, 10, 10), 13)
    okp = (dy.data_ptr(), dx.data_ptr()) + ptrs + (24, 3, 8, 8, 1)
    assert pad(*okp) == 0
    torch.cuda.synchronize()
    for i in range(5):
        assert pad(*(okp[:i] + (None,) + okp[i + 1:])) == -1
    assert pad(*(okp[:9] + (9,))) == -1                                          # padding larger than the face
    assert pad(*(okp[:9] + (0,))) == -1
    assert pad(*(okp[:5] + (13,) + okp[6:])) == -1
    assert pad(*(okp[:7] + (8, 9) + okp[9:])) == -1
