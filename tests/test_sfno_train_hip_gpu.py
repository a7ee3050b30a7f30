"""Training SFNO2DModule on the HIP backwards of csrc/sht.hip: parameter gradients of a 2-step `.train()` rollout against the
float64 network of tests/sht_ref.py, at the two configurations tests/test_sfno_gpu.py does not differentiate -- a middle block
on the inner grid (three layers) and differing forward / inverse grids (scale_factor 2), where the residual of a block goes
through inv(c) and so through a second inverse transform's backward.  Bound: 1e-6 relative, the project's training bound; the
measured worst case stands in DESIGN.md section 35.7.

The backward has no atomics: a second run from the same state gives the same bits.  That comparison runs with the
convolutions' gradients on the project's own kernels (DLWP_CONV_DGRAD=hip, DLWP_CONV_WGRAD=hip: "bit-reproducible gradients",
training.conv_dgrad_mode), because the library's convolution weight gradient, which the default path calls for the 1x1
layers, is not reproducible from call to call: measured inside the whole suite, the gradient of blocks.0.inner_skip.weight
(torch.ops.aten.convolution_backward) differed between two runs while every gradient that had passed through ALL of the
transforms' and the mix's backwards before it (encoder.0.weight, encoder.0.bias, encoder.2.weight,
blocks.0.filter.filter.weight) was bit-identical.
"""
import pytest
import torch

import sht_ref as R
from dlwp_benchmark_amd import training as T
from dlwp_benchmark_amd.models import SFNO2DModule
from dlwp_benchmark_amd.weights import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHANNELS = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=3)
CASES = {
    "lg8x16-3layers-ctx2": dict(height=8, width=16, grid="legendre-gauss", num_layers=3, scale_factor=1, context_size=2,
                                use_mlp=False, big_skip=False, pos_embed=False, activation_function="relu"),
    "lg16x32-scale2": dict(height=16, width=32, grid="legendre-gauss", num_layers=3, scale_factor=2, context_size=1, use_mlp=False,
                           big_skip=True, pos_embed=False),
}


def _std(name, shape):
    return 0.7 / shape[0] ** 0.5 if name.endswith("filter.filter.weight") else None      # one complex [in, out] matrix per degree


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float(torch.linalg.vector_norm(a.double() - b) / torch.linalg.vector_norm(b))


@pytest.mark.parametrize("case", sorted(CASES))
def test_training_gradients_on_the_hip_backward_against_float64(case, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the torch form was differentiated on the default path")

    monkeypatch.delenv("DLWP_TRAIN_TORCH_BACKWARD", raising=False)
    monkeypatch.setattr(T, "_grad_of_torch_form", refuse)
    kw = dict(CASES[case], embed_dim=16, **CHANNELS)
    model = SFNO2DModule(**kw)
    fill_state_dict(model, std_fn=_std)
    params = {k[len("sfno."):]: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(5)
    h, w, ctx = kw["height"], kw["width"], kw["context_size"]
    const = torch.randn(2, 1, 2, h, w, generator=g)
    presc = torch.randn(2, ctx + 2, 1, h, w, generator=g)
    prog = torch.randn(2, ctx + 2, 3, h, w, generator=g)
    cot = torch.randn(2, 2, 3, h, w, generator=g)

    def gradients():
        model.zero_grad(set_to_none=True)
        out = model(constants=const.to(DEV), prescribed=presc.to(DEV), prognostic=prog.to(DEV))
        assert out.requires_grad
        (out * cot.to(DEV)).sum().backward()
        return out.detach(), {name: p.grad.clone() for name, p in model.named_parameters()}

    out, grads = gradients()
    want = R.SfnoRef(params, **kw).rollout(const.double(), presc.double(), prog.double())
    assert _rel(out.cpu(), want.detach()) <= 1e-5
    (want * cot.double()).sum().backward()
    worst = 0.0
    for name, got in grads.items():
        err = _rel(got.cpu(), params[name[len("sfno."):]].grad)
        worst = max(worst, err)
        print(f"{case} grad {name}: {err:.3e}")
    print(f"{case}: worst parameter gradient {worst:.3e}")
    assert worst <= 1e-6
    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    monkeypatch.setenv("DLWP_CONV_WGRAD", "hip")
    _, first = gradients()
    _, again = gradients()
    for name, got in first.items():
        assert torch.equal(got, again[name]), name
