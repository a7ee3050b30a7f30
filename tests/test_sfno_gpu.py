"""SFNO2DModule (dlwp_benchmark_amd/models/sfno.py) against the float64 network of tests/sht_ref.py.

PARITY UNPINNED at the library boundary (torch_harmonics is not available): what is checked is that the HIP path computes the
network the module documents.  Weights come from weights.normal (through fill_state_dict) and are copied into both.  Bounds:
rel-L2 <= 1e-5 per rollout step (the project's fp32 bound of every backbone), 1e-6 relative for the parameter gradients (the
project's training bound), bitwise equality for the captured-step and chunked paths.
"""
import numpy as np
import pytest
import torch

import sht_ref as R
from dlwp_benchmark_amd.models import SFNO2DModule
from dlwp_benchmark_amd.rollout import rollout_chunks
from dlwp_benchmark_amd.weights import fill_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHANNELS = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=3)

# E = 16 throughout.  num_layers 3 has a middle block on the inner grid; scale_factor 2 recomputes the residual of block 0 on
# the inner grid; use_mlp, big_skip and pos_embed appear both ways; context 1 and 2; both activations; both quadratures.
CASES = {
    "lg8x16-2layers": dict(height=8, width=16, grid="legendre-gauss", num_layers=2, scale_factor=1, context_size=1, use_mlp=True,
                           big_skip=True, pos_embed=True),
    "lg8x16-3layers-ctx2": dict(height=8, width=16, grid="legendre-gauss", num_layers=3, scale_factor=1, context_size=2,
                                use_mlp=False, big_skip=False, pos_embed=False, activation_function="relu"),
    "eq32x64": dict(height=32, width=64, grid="equiangular", num_layers=2, scale_factor=1, context_size=1, use_mlp=True,
                    big_skip=False, pos_embed=True),
    "lg16x32-scale2": dict(height=16, width=32, grid="legendre-gauss", num_layers=3, scale_factor=2, context_size=1, use_mlp=False,
                           big_skip=True, pos_embed=False),
}


def _std(name, shape):
    if name.endswith("filter.filter.weight"):
        return 0.7 / shape[0] ** 0.5             # one complex [in, out] matrix per degree
    if name.endswith("pos_embed"):
        return 0.5
    return None


def _build(case: str):
    kw = dict(CASES[case], embed_dim=16, **CHANNELS)
    model = SFNO2DModule(**kw)
    fill_state_dict(model, std_fn=_std)
    params = {k[len("sfno."):]: v.detach().double().clone() for k, v in model.state_dict().items()}
    return model.to(DEV), params, kw


def _inputs(kw, batch=2, steps=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    h, w, ctx = kw["height"], kw["width"], kw["context_size"]
    const = torch.randn(batch, 1, kw["constant_channels"], h, w, generator=g)
    presc = torch.randn(batch, ctx + steps, kw["prescribed_channels"], h, w, generator=g)
    prog = torch.randn(batch, ctx + steps, kw["prognostic_channels"], h, w, generator=g)
    return const, presc, prog


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float(torch.linalg.vector_norm(a.double() - b) / torch.linalg.vector_norm(b))


@pytest.mark.parametrize("case", sorted(CASES))
def test_rollout_against_float64(case):
    model, params, kw = _build(case)
    model.eval()
    const, presc, prog = _inputs(kw)
    with torch.no_grad():
        want = R.SfnoRef(params, **kw).rollout(const.double(), presc.double(), prog.double())
    got = model(constants=const.to(DEV), prescribed=presc.to(DEV), prognostic=prog.to(DEV))
    assert got.is_cuda and tuple(got.shape) == tuple(want.shape) == (2, 4, 3, kw["height"], kw["width"])
    errs = [_rel(got[:, s].cpu(), want[:, s]) for s in range(4)]
    print(f"{case}: rel-L2 per step {', '.join(f'{e:.2e}' for e in errs)}")
    assert max(errs) <= 1e-5
    # the increments are not small beside the state: the check is not carried by the residual path
    assert _rel(prog[:, kw["context_size"] - 1].double(), want[:, 0]) > 0.05


def test_step_graphs_and_chunks_are_bitwise_the_eager_rollout():
    model, _, kw = _build("lg8x16-2layers")
    model.eval()
    const, presc, prog = (t.to(DEV) for t in _inputs(kw))
    eager = model(constants=const, prescribed=presc, prognostic=prog).clone()
    model.set_step_graphs(True)
    graphed = model(constants=const, prescribed=presc, prognostic=prog).clone()
    model.set_step_graphs(False)
    assert torch.equal(eager, graphed)
    parts = [(s0, out.clone()) for s0, out in rollout_chunks(model, const, presc, prog[:, :kw["context_size"]], 4, 2)]
    assert [s0 for s0, _ in parts] == [0, 2]
    assert torch.equal(torch.cat([o for _, o in parts], dim=1), eager)


def test_training_gradients_against_float64():
    model, params, kw = _build("lg8x16-2layers")
    model.train()
    const, presc, prog = _inputs(kw, steps=2)
    cot = torch.randn(2, 2, 3, kw["height"], kw["width"], generator=torch.Generator().manual_seed(9))
    out = model(constants=const.to(DEV), prescribed=presc.to(DEV), prognostic=prog.to(DEV))
    assert out.requires_grad
    (out * cot.to(DEV)).sum().backward()
    ref_params = {k: v.requires_grad_(True) for k, v in params.items()}
    want = R.SfnoRef(ref_params, **kw).rollout(const.double(), presc.double(), prog.double())
    assert _rel(out.detach().cpu(), want.detach()) <= 1e-5
    (want * cot.double()).sum().backward()
    worst = 0.0
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        err = _rel(p.grad.cpu(), ref_params[name[len("sfno."):]].grad)
        worst = max(worst, err)
        print(f"grad {name}: {err:.3e}")
    assert worst <= 1e-6


def test_one_step_stays_on_the_device_and_checks_its_input():
    from dlwp_benchmark_amd.lib import DlwpError

    model, _, kw = _build("lg8x16-3layers-ctx2")
    model.eval()
    x = torch.randn(2, model.in_channels, 8, 16, device=DEV)
    with torch.no_grad():
        y = model.one_step(x)
    assert y.is_cuda and tuple(y.shape) == (2, 3, 8, 16)
    with pytest.raises(DlwpError):
        model.one_step(torch.randn(2, model.in_channels + 1, 8, 16, device=DEV))
    with pytest.raises(DlwpError):
        model.one_step(torch.randn(2, model.in_channels, 16, 16, device=DEV))
