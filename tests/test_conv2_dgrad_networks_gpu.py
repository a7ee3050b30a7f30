"""Whole training steps of the U-Net family with no library convolution at all: DLWP_CONV_DGRAD=hip and DLWP_CONV_WGRAD=hip,
every library form the step could still reach replaced by a function that raises.

  * the drivers of test_training_gpu.py (UNet) and test_hpx_train_gpu.py (UNetHPX, MUNetHPX) hold their own bounds against the
    real classes' fixtures -- loss 1e-5, gradients 1e-4 -- with the forward of the non-3x3 layers now the "bf16x6" form;
  * "hip" against "torch" on MUNetHPX and on a tiny DiffModernUNet.single_forward step: per-parameter rel-L2 <= 1e-5, the bound of
    test_hip_and_torch_paths_agree;
  * with the variable unset, spies on the new ops see no call."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARY_FORMS = ("conv2d_torch", "conv_transpose2d_torch", "conv2d_input_grad_torch", "conv2d_weight_grad_torch",
                 "conv3x3_weight_grad_torch")
NEW_OPS = ("conv2d_input_grad", "conv_transpose2d_input_grad", "avgpool2x2_backward")


def _raiser(name):
    def f(*a, **kw):
        shapes = [tuple(t.shape) for t in a if isinstance(t, torch.Tensor)]
        raise AssertionError(f"{name} was called under DLWP_CONV_DGRAD=hip: tensors {shapes}, arguments "
                             f"{[v for v in a if not isinstance(v, torch.Tensor)]} {kw}")
    return f


def no_library_convolution(monkeypatch):
    from dlwp_benchmark_amd import training

    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    monkeypatch.setenv("DLWP_CONV_WGRAD", "hip")
    for name in LIBRARY_FORMS:
        monkeypatch.setattr(training, name, _raiser("training." + name))
    monkeypatch.setattr(F, "conv_transpose2d", _raiser("F.conv_transpose2d"))
    monkeypatch.setattr(F, "avg_pool2d", _raiser("F.avg_pool2d"))


def test_unet_gradients_match_reference(monkeypatch):
    from test_training_gpu import test_training_gradients_match_reference as driver

    no_library_convolution(monkeypatch)
    driver("unet_h4_32x64")


@pytest.mark.parametrize("tag", ["unethpx_h4_8x8", "munethpx_h16_8_norm"])
def test_hpx_gradients_match_reference(tag, monkeypatch):
    from dlwp_benchmark_amd import training
    from test_hpx_train_gpu import test_hpx_gradients_match_reference as driver

    no_library_convolution(monkeypatch)
    monkeypatch.setattr(training, "HPX_DX_DIRECT_MAX_COUT", 0)         # every HEALPix input gradient through the two-step form
    driver(tag)


def _munethpx_grads():
    from test_hpx_train_gpu import _step

    _, model, loss = _step("munethpx_h16_8_norm")
    return float(loss), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _diffmodernunet_grads():
    """one train.py-style single_forward step of a tiny DiffModernUNet (8 x 16, hidden [8, 16], no attention)"""
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd import weights as W

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_diffusion_attention_grad as dtool
    finally:
        sys.path.pop(0)
    cfg = dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[8, 16], context_size=1,
               norm=True, attention=False, num_refinement_step=2)
    model = M.DiffModernUNet(**cfg)
    W.fill_state_dict(model, gain=0.7)
    model = model.to(DEV).train()
    tag = "conv2_dgrad_diffmodernunet"
    args = {a: W.normal(n, s, 1.0).to(DEV) for a, n, s in dtool.net_inputs(tag, "DiffModernUNet", cfg, 2, (8, 16))}
    case = dict(kwargs=cfg, betas=[0.4, 0.2, 0.1], k=1, noise=f"golden/diffattn_grad/{tag}/noise")
    loss = dtool.train_step_loss(model, args, case)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("step", [_munethpx_grads, _diffmodernunet_grads], ids=["munethpx_h16_8_norm", "diffmodernunet_8x16"])
def test_hip_agrees_with_torch(step, monkeypatch):
    monkeypatch.setenv("DLWP_CONV_DGRAD", "torch")
    monkeypatch.setenv("DLWP_CONV_WGRAD", "hip")
    loss_t, ref = step()
    no_library_convolution(monkeypatch)
    loss_h, got = step()
    assert set(got) == set(ref) and len(ref) > 0
    worst = max(rel_l2(got[n], ref[n]) for n in ref)
    print("hip against torch: loss %.2e, worst parameter gradient rel-L2 %.2e" % (abs(loss_h - loss_t) / abs(loss_t), worst))
    assert abs(loss_h - loss_t) <= 1e-5 * abs(loss_t)
    for n in ref:
        assert rel_l2(got[n], ref[n]) <= 1e-5, n


def test_unset_switch_calls_no_new_op(monkeypatch):
    from dlwp_benchmark_amd import ops

    monkeypatch.delenv("DLWP_CONV_DGRAD", raising=False)
    for name in NEW_OPS:
        monkeypatch.setattr(ops, name, _raiser("ops." + name))
    _munethpx_grads()
    _diffmodernunet_grads()
