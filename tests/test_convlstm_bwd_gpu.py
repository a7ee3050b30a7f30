"""dlwp_convlstm_gates_bwd_f32 (csrc/convlstm_bwd.hip) against float64 autograd of the cell update, the autograd Function
around it (training.convlstm_gates), and ConvLSTM / ConvLSTMHPX trained through it against the gradients the real reference
classes produced (tests/golden/grad_convlstm_h8_32x64.npz, grad_hpx_convlstmhpx_h8_8x8.npz)."""
import json

import pytest
import torch

from helpers import load_golden, rel_l2
from test_convlstm_bwd_cpu import saturated_gates

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the shapes of test_convlstm_gates_match_float64 -- odd everything (one pixel per thread), below the grid cap, at 2^20 elements
# and odd past the cap of 256 * 8 workgroups -- and one more past the cap in the four-pixel form, which divides the work by 4
SHAPES = [(3, 5, 7, 9), (2, 8, 32, 64), (32, 16, 32, 64), (5, 24, 61, 127), (34, 32, 32, 64)]


def _inputs(b, hid, H, W):
    g = torch.Generator(device=DEV).manual_seed(b * hid + H)
    gates = saturated_gates((b, 4 * hid, H, W), g, device=DEV)
    c_prev = torch.randn(b, hid, H, W, device=DEV, generator=g) * 2.0
    dh = torch.randn(b, hid, H, W, device=DEV, generator=g)
    dc = torch.randn(b, hid, H, W, device=DEV, generator=g)
    return gates, c_prev, dh, dc


def _float64_autograd(gates, c_prev, dh, dc):
    from dlwp_benchmark_amd import training as T

    g_ = gates.double().requires_grad_(True)
    c_ = c_prev.double().requires_grad_(True)
    h, c = T.convlstm_gates_torch(g_, c_)
    return torch.autograd.grad([h, c], [g_, c_], [dh.double(), dc.double()])


@pytest.mark.parametrize("b,hid,H,W", SHAPES)
def test_kernel_matches_float64_autograd(b, hid, H, W):
    """rel-L2 <= 1e-6 and |got - want| <= 1e-6 (|dh| + |dc|) (1 + |c_prev|) per element: the bound the forward is held to on
    these inputs; an fp32 evaluation of the closed form with an emulated __expf sits at 1.6e-7 / 5.5e-8 rel-L2"""
    from dlwp_benchmark_amd import ops

    gates, c_prev, dh, dc = _inputs(b, hid, H, W)
    dgates, dc_prev = ops.convlstm_gates_backward(gates, c_prev, dh, dc)
    want_g, want_c = _float64_autograd(gates, c_prev, dh, dc)
    assert dgates.shape == gates.shape and dc_prev.shape == c_prev.shape
    assert torch.isfinite(dgates).all() and torch.isfinite(dc_prev).all()
    scale = 1e-6 * (dh.double().abs() + dc.double().abs()) * (1.0 + c_prev.double().abs())
    for got, want, bound, tag in ((dgates, want_g, scale.repeat(1, 4, 1, 1), "dgates"), (dc_prev, want_c, scale, "dc_prev")):
        err = rel_l2(got, want)
        worst = float(((got.double() - want).abs() / bound).max())
        print(f"gates bwd {b}x{hid}x{H}x{W} {tag}: rel-L2 {err:.3e}, worst element at {worst:.3f} of its bound")
        assert err <= 1e-6, (tag, err)
        assert ((got.double() - want).abs() <= bound).all(), tag


@pytest.mark.parametrize("b,hid,H,W", [(3, 5, 7, 9), (2, 8, 32, 64)])
def test_missing_arguments_equal_zero_tensors_and_reruns_are_bitwise(b, hid, H, W):
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.lib import DlwpError

    gates, c_prev, dh, dc = _inputs(b, hid, H, W)
    zero = torch.zeros_like(c_prev)
    full = ops.convlstm_gates_backward(gates, c_prev, dh, dc)
    again = ops.convlstm_gates_backward(gates, c_prev, dh, dc)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])
    for got, want in ((ops.convlstm_gates_backward(gates, c_prev, dh, None), ops.convlstm_gates_backward(gates, c_prev, dh, zero)),
                      (ops.convlstm_gates_backward(gates, c_prev, None, dc), ops.convlstm_gates_backward(gates, c_prev, zero, dc))):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    dg, none = ops.convlstm_gates_backward(gates, c_prev, dh, dc, need_c_prev=False)
    assert none is None and torch.equal(dg, full[0])
    with pytest.raises(DlwpError, match="neither"):
        ops.convlstm_gates_backward(gates, c_prev, None, None)


def test_unaligned_tensors_take_the_one_pixel_form():
    """H * W a multiple of 4 but storage 4 bytes off a 16-byte boundary: the same bits as the aligned call"""
    from dlwp_benchmark_amd import ops

    gates, c_prev, dh, dc = _inputs(2, 8, 32, 64)
    want = ops.convlstm_gates_backward(gates, c_prev, dh, dc)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        buf[1:].copy_(t.reshape(-1))
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    got = ops.convlstm_gates_backward(shifted(gates), shifted(c_prev), shifted(dh), shifted(dc))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_function_runs_the_kernels_in_both_directions(monkeypatch):
    from dlwp_benchmark_amd import ops, training as T

    gates, c_prev, dh, dc = _inputs(2, 8, 32, 64)
    with torch.no_grad():
        h0, c0 = ops.convlstm_gates(gates, c_prev)
    g_, c_ = gates.clone().requires_grad_(True), c_prev.clone().requires_grad_(True)
    h, c = T.convlstm_gates(g_, c_)
    assert h.requires_grad and c.requires_grad and torch.equal(h, h0) and torch.equal(c, c0)
    h2, c2 = ops.convlstm_gates(g_, c_)                  # the public op sends the gradient case the same way
    assert h2.requires_grad and torch.equal(h2, h0) and torch.equal(c2, c0)
    got = torch.autograd.grad([h, c], [g_, c_], [dh, dc], retain_graph=True)
    want = ops.convlstm_gates_backward(gates, c_prev, dh, dc)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a gradient autograd does not have reaches the kernel as a null pointer; an input that takes none is not computed
    only_h = torch.autograd.grad([h], [g_, c_], [dh], retain_graph=True)
    want_h = ops.convlstm_gates_backward(gates, c_prev, dh, None)
    assert torch.equal(only_h[0], want_h[0]) and torch.equal(only_h[1], want_h[1])
    h3, c3 = T.convlstm_gates(g_, c_prev)
    assert torch.equal(torch.autograd.grad([h3, c3], [g_], [dh, dc])[0], want[0])
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    ht, ct = T.convlstm_gates(g_, c_)
    ref = torch.autograd.grad([ht, ct], [g_, c_], [dh, dc])
    for a, r, tag in ((got[0], ref[0], "dgates"), (got[1], ref[1], "dc_prev")):
        err = rel_l2(a, r)
        print(f"HIP backward against autograd of the torch chain, {tag}: rel-L2 {err:.3e}")
        assert err <= 1e-5, tag


# ---- the networks, on the fixtures of test_training_gpu.py and test_hpx_train_gpu.py -------------------------------------------
LATLON, HPX = "convlstm_h8_32x64", "convlstmhpx_h8_8x8"


def _latlon_step(tag):
    """the fixture's ConvLSTM on the GPU in train mode, one rollout-MSE backward (the loading code of
    test_training_gradients_match_reference); returns (fixture, model, loss)"""
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.make_golden import GRAD_CASES, MODEL_CASES, model_inputs, rollout_mse

    base, frames = GRAD_CASES[tag]
    family, cfg, (batch, _), gain = MODEL_CASES[base]
    assert family == "convlstm"
    g = load_golden(f"grad_{tag}")
    model = M.ConvLSTM(**cfg)
    assert fill_state_dict(model, gain=gain) == str(g["sha"]), "filler drifted: regenerate fixtures"
    model = model.to(DEV).train()
    dev = lambda t: t.to(DEV) if t is not None else None
    constants, prescribed, prognostic = [dev(t) for t in model_inputs(base, cfg, batch, frames)]
    y = model(constants=constants, prescribed=prescribed, prognostic=prognostic)
    assert y.requires_grad
    loss = rollout_mse(y, prognostic, cfg["context_size"])
    loss.backward()
    torch.cuda.synchronize()
    return g, model, loss


def _step(tag):
    if tag == LATLON:
        from oracle.make_golden import grad_probe

        return (*_latlon_step(tag), grad_probe)
    from test_hpx_train_gpu import _step as hpx_step, _tool

    return (*hpx_step(tag), _tool().grad_probe)


def _worst_deviation(g, model, tag, grad_probe):
    """the measure of test_training_gradients_match_reference / test_hpx_gradients_match_reference"""
    params = dict(model.named_parameters())
    worst = 0.0
    for i, pname in enumerate(json.loads(str(g["names"]))):
        assert pname in params and params[pname].grad is not None, f"no gradient for {pname}"
        gr = params[pname].grad.detach().double().cpu()
        n_ref, p_ref = float(g["norms"][i]), float(g["projs"][i])
        scale = max(n_ref, 1e-12)
        worst = max(worst, abs(float(gr.norm()) - n_ref) / scale)
        r = grad_probe(tag, pname, gr.shape).double()
        worst = max(worst, abs(float((gr * r).sum()) - p_ref) / (scale * float(r.norm())))
    for key in g.files:
        if key.startswith("grad::"):
            want = torch.from_numpy(g[key]).double()
            got = params[key[6:]].grad.detach().double().cpu()
            worst = max(worst, float((got - want).norm() / want.norm().clamp_min(1e-30)))
    return worst


@pytest.mark.parametrize("tag", [LATLON, HPX])
def test_networks_train_on_the_kernel_alone(tag, monkeypatch):
    """with the torch chain and torch.sigmoid raising, the train step completes and meets the fixtures' bounds"""
    from dlwp_benchmark_amd import training as T

    def boom(*a, **k):
        raise AssertionError("the ConvLSTM cell ran torch operators under training")

    monkeypatch.setattr(T, "convlstm_gates_torch", boom)
    monkeypatch.setattr(torch, "sigmoid", boom)
    g, model, loss, probe = _step(tag)
    dl = abs(float(loss) - float(g["loss"])) / abs(float(g["loss"]))
    worst = _worst_deviation(g, model, tag, probe)
    print(f"{tag}: loss deviation {dl:.2e}, worst gradient deviation {worst:.2e}")
    assert dl <= 1e-5 and worst <= 1e-4


@pytest.mark.parametrize("tag", [LATLON, HPX])
def test_networks_agree_with_the_torch_backward(tag, monkeypatch):
    _, hip, _, _ = _step(tag)
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    _, ref, _, _ = _step(tag)
    worst = 0.0
    for (name, a), (_, b) in zip(hip.named_parameters(), ref.named_parameters()):
        err = rel_l2(a.grad, b.grad)
        worst = max(worst, err)
        assert err <= 1e-5, name
    print(f"{tag}: worst parameter gradient against DLWP_TRAIN_TORCH_BACKWARD=1: rel-L2 {worst:.2e}")
