"""The torch forms of the ConvLSTM cell and of its backward (training.convlstm_gates_torch, convlstm_gates_backward_torch) on
the CPU in float64: the closed form dlwp_convlstm_gates_bwd_f32 evaluates against autograd of the operator chain."""
import pytest
import torch

from helpers import rel_l2


def saturated_gates(shape, g, device="cpu", dtype=torch.float32):
    """standard-normal gate inputs at scale 4 with a fifth replaced by +-30 / +-90 (the mix of
    test_convlstm_gates_match_float64: where __expf saturates, or overflows to inf)"""
    gates = torch.randn(*shape, device=device, generator=g, dtype=dtype) * 4.0
    pick = torch.rand(shape, device=device, generator=g)
    sat = torch.where(torch.rand(shape, device=device, generator=g) < 0.5, 30.0, 90.0)
    sat = torch.where(torch.rand(shape, device=device, generator=g) < 0.5, sat, -sat)
    return torch.where(pick < 0.2, sat.to(dtype), gates)


def _case(seed=0, shape=(3, 5, 7, 9)):
    b, hid, h, w = shape
    g = torch.Generator().manual_seed(seed)
    gates = saturated_gates((b, 4 * hid, h, w), g, dtype=torch.float64)
    c_prev = torch.randn(b, hid, h, w, generator=g, dtype=torch.float64) * 2.0
    dh = torch.randn(b, hid, h, w, generator=g, dtype=torch.float64)
    dc = torch.randn(b, hid, h, w, generator=g, dtype=torch.float64)
    return gates, c_prev, dh, dc


def test_closed_form_matches_float64_autograd():
    from dlwp_benchmark_amd import training as T

    gates, c_prev, dh, dc = _case()
    g_ = gates.clone().requires_grad_(True)
    c_ = c_prev.clone().requires_grad_(True)
    h, c = T.convlstm_gates_torch(g_, c_)
    want_g, want_c = torch.autograd.grad([h, c], [g_, c_], [dh, dc])
    got_g, got_c = T.convlstm_gates_backward_torch(gates, c_prev, dh, dc)
    assert got_g.dtype == torch.float64 and got_g.shape == gates.shape and got_c.shape == c_prev.shape
    assert torch.isfinite(got_g).all() and torch.isfinite(got_c).all()
    eg, ec = rel_l2(got_g, want_g), rel_l2(got_c, want_c)
    print(f"closed form against float64 autograd: dgates {eg:.3e}, dc_prev {ec:.3e}")
    assert eg <= 1e-12 and ec <= 1e-12


@pytest.mark.parametrize("missing", ["dh", "dc"])
def test_missing_gradient_is_a_zero_gradient(missing):
    from dlwp_benchmark_amd import training as T

    gates, c_prev, dh, dc = _case(seed=1)
    zero = torch.zeros_like(c_prev)
    if missing == "dh":
        got, want = T.convlstm_gates_backward_torch(gates, c_prev, None, dc), T.convlstm_gates_backward_torch(gates, c_prev, zero, dc)
    else:
        got, want = T.convlstm_gates_backward_torch(gates, c_prev, dh, None), T.convlstm_gates_backward_torch(gates, c_prev, dh, zero)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_both_gradients_missing_is_refused():
    from dlwp_benchmark_amd import training as T
    from dlwp_benchmark_amd.lib import DlwpError

    gates, c_prev, _, _ = _case(seed=2)
    with pytest.raises(DlwpError, match="neither"):
        T.convlstm_gates_backward_torch(gates, c_prev, None, None)


def test_torch_form_is_the_cell_formula():
    """convlstm_gates_torch against convlstm.py:96-109 written out in float64"""
    from dlwp_benchmark_amd import training as T

    gates, c_prev, _, _ = _case(seed=3)
    h, c = T.convlstm_gates_torch(gates, c_prev)
    netin, ig, fg, og = torch.split(gates, gates.shape[1] // 4, dim=1)
    sig = lambda t: 1.0 / (1.0 + torch.exp(-t))
    c_want = sig(fg) * c_prev + sig(ig) * torch.tanh(netin)
    h_want = sig(og) * torch.tanh(c_want)
    assert torch.isfinite(h).all() and torch.isfinite(c).all()
    assert rel_l2(c, c_want) <= 1e-12 and rel_l2(h, h_want) <= 1e-12
    # and in float32 on the CPU: the chain ops.convlstm_gates used to build under autograd, on any dtype
    h32, c32 = T.convlstm_gates_torch(gates.float(), c_prev.float())
    assert h32.dtype == torch.float32 and rel_l2(c32, c_want) <= 1e-6 and rel_l2(h32, h_want) <= 1e-6


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """dlwp_convlstm_gates_bwd_f32 validates on the host: both gradients missing, a bad shape and an output that aliases an
    input are DLWP_ERR_INVALID_ARGUMENT (-1), answered without a device (the addresses are never dereferenced)"""
    from dlwp_benchmark_amd import lib as L

    fn = L.load().dlwp_convlstm_gates_bwd_f32
    gates, c_prev, dh, dc, dgates, dc_prev = (0x1000 * (i + 1) for i in range(6))
    for args, why in (((gates, c_prev, None, None, dgates, dc_prev, 2, 4, 8, 16), "neither"),
                      ((gates, c_prev, dh, dc, None, dc_prev, 2, 4, 8, 16), "null"),
                      ((gates, c_prev, dh, dc, dgates, dc_prev, 2, 0, 8, 16), "shape"),
                      ((gates, c_prev, dh, dc, gates, dc_prev, 2, 4, 8, 16), "alias"),
                      ((gates, c_prev, dh, dc, dgates, dc, 2, 4, 8, 16), "alias"),
                      ((gates, c_prev, dh, dc, dgates, dgates, 2, 4, 8, 16), "alias")):
        assert fn(*args, None) == -1, args
        assert why in L.load().dlwp_last_error().decode(), (why, L.load().dlwp_last_error())
