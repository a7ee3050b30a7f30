"""MeshGraphNet on the GPU (csrc/mgn.hip through ops.mgn_mlp / ops.mgn_processor_layer): rollouts and a gradient against the
REAL reference class (tests/golden/mgn_*.npz, tools/make_golden_meshgraphnet.py), the fused processor layer against an fp64
restatement on irregular graphs, determinism, step-graph replay, no torch fall-back on supported shapes, the fall-back
beyond the envelope, and the memory bound."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden, per_step_rel_l2, rel_l2

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUTS = ["yaml_delaunay_32x64", "grid_mean_mp2_16x16", "stencil8_16x32", "default_widths_delaunay_8x16",
            "d470_delaunay_8x16", "ctx2_prescribed_grid_8x16", "grid_nonperiodic_8x16"]


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_meshgraphnet as t
    finally:
        sys.path.pop(0)
    return t


def _model(g, tool):
    from dlwp_benchmark_amd.models import MeshGraphNet

    case = json.loads(str(g["case"]))
    h, w, periodic = case["graph"]
    m = MeshGraphNet(**case["kwargs"], graph=dict(height=h, width=w, periodic=periodic))
    assert tool.fill(m) == str(g["sha"])
    m.invalidate_packed()
    m.set_fused_layers("always")            # the kernels at every width of the fixtures, 128 and 470 included
    return m.to(DEV).eval(), case


def _inputs(tool, tag, case, dev=DEV):
    c, p, q = tool.case_inputs(tag, case["kwargs"], case["batch"], case["frames"], case["graph"][:2])
    return [t.to(dev) if t is not None else None for t in (c, p, q)]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ROLLOUTS)
def test_rollout_matches_reference_golden(tag):
    tool = _tool()
    g = load_golden(f"mgn_rollout_{tag}")
    m, case = _model(g, tool)
    assert m.uses_fused_layers()
    c, p, q = _inputs(tool, tag, case)
    y = m(constants=c, prescribed=p, prognostic=q)
    torch.cuda.synchronize()
    want = torch.from_numpy(g["y"])
    assert y.shape == want.shape
    errs = per_step_rel_l2(y, want)
    assert max(errs) <= 1e-5, f"{tag}: per-step rel L2 {errs}"


@pytest.mark.gpu
def test_gradient_matches_reference_golden():
    tool = _tool()
    g = load_golden("mgn_grad_yaml_8x16")
    m, case = _model(g, tool)
    m.train()
    c, p, q = _inputs(tool, "grad_yaml_8x16", case)
    y = m(constants=c, prescribed=p, prognostic=q)
    ctx = case["kwargs"]["context_size"]
    loss = torch.mean((y - q[:, ctx:]) ** 2)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    names = json.loads(str(g["names"]))
    params = dict(m.named_parameters())
    norms, projs = [], []
    for name in names:
        gr = params[name].grad.detach().double().cpu()
        norms.append(float(gr.norm()))
        projs.append(float((gr * tool.W.normal(f"golden/mgn/grad_yaml_8x16/probe/{name}", tuple(gr.shape), 1.0).double()).sum()))
    np.testing.assert_allclose(norms, g["norms"], rtol=1e-4, atol=1e-4 * float(np.max(g["norms"])))
    np.testing.assert_allclose(projs, g["projs"], rtol=1e-4, atol=1e-4 * float(np.max(np.abs(g["projs"]))))


def _random_graph(n, seed):
    gen = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 13, (n,), generator=gen)
    deg[::7] = 0                                             # isolated nodes
    src = torch.randint(0, n, (int(deg.sum()),), generator=gen).int()
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).int()
    dst = torch.repeat_interleave(torch.arange(n), deg).int()
    return row_ptr, src, dst, deg.int()


LAYER_CASES = [(1, 1, "sum"), (34, 2, "sum"), (34, 4, "mean"), (64, 3, "mean"), (128, 2, "sum"), (128, 1, "mean"),
               (470, 2, "sum"), (512, 4, "mean"), (512, 1, "sum")]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,depth,agg", LAYER_CASES)
def test_processor_layer_matches_fp64_restatement(dim, depth, agg):
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    torch.manual_seed(dim * 10 + depth)
    n, b = 97, 3
    row_ptr, src, dst, deg = _random_graph(n, dim + depth)
    ne = src.numel()
    em, nm = MeshGraphMLP(3 * dim, dim, dim, depth), MeshGraphMLP(2 * dim, dim, dim, depth)
    for p in list(em.parameters()) + list(nm.parameters()):
        with torch.no_grad():
            p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 5.0))
    with torch.no_grad():
        em.model[-1].weight.add_(1.0)                            # LayerNorm scales around 1
        nm.model[-1].weight.add_(1.0)
    x = torch.randn(b * n, dim)
    for shared in (True, False):
        e = torch.randn(ne, dim) if shared else torch.randn(b * ne, dim)
        want_x, want_e = ops.mgn_layer_torch(em.double().model, nm.double().model, agg, src, dst, deg, b, x.double(),
                                             e.double())
        em.float(), nm.float()
        emd, nmd = em.to(DEV), nm.to(DEV)
        x_out = torch.empty(b * n, dim, device=DEV)
        e_out = torch.empty(b * ne, dim, device=DEV) if shared else e.to(DEV)      # in place when per-sample
        ops.mgn_processor_layer(ops.MgnMlpWeights(), emd.model, ops.MgnMlpWeights(), nmd.model, agg, row_ptr.to(DEV),
                                src.to(DEV), dst.to(DEV), b, x.to(DEV), x_out, e.to(DEV) if shared else e_out, shared, e_out)
        torch.cuda.synchronize()
        em, nm = emd.cpu(), nmd.cpu()
        assert rel_l2(x_out, want_x) <= 1e-5, (dim, depth, agg, shared, rel_l2(x_out, want_x))
        assert rel_l2(e_out, want_e) <= 1e-5, (dim, depth, agg, shared, rel_l2(e_out, want_e))


@pytest.mark.gpu
def test_shared_edge_table_may_not_be_overwritten():
    from dlwp_benchmark_amd import lib, ops
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    row_ptr, src, dst, _ = _random_graph(16, 0)
    em, nm = MeshGraphMLP(12, 4, 4, 1).to(DEV), MeshGraphMLP(8, 4, 4, 1).to(DEV)
    x, e = torch.randn(16, 4, device=DEV), torch.randn(src.numel(), 4, device=DEV)
    with pytest.raises(lib.DlwpError):
        ops.mgn_processor_layer(ops.MgnMlpWeights(), em.model, ops.MgnMlpWeights(), nm.model, "sum", row_ptr.to(DEV),
                                src.to(DEV), dst.to(DEV), 1, x, torch.empty_like(x), e, True, e)


@pytest.mark.gpu
def test_strided_channels_first_input_is_read_correctly():
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    torch.manual_seed(3)
    m = MeshGraphMLP(5, 96, 80, 2).to(DEV)
    x = torch.randn(2, 4, 6, 5, device=DEV).permute(0, 3, 1, 2)          # [B, C, H, W], not contiguous
    y = ops.mgn_mlp(ops.MgnMlpWeights(), m.model, x, 2, 24, channels_first_in=True)
    want = m.double()(x.double().permute(0, 2, 3, 1).reshape(48, 5))
    assert rel_l2(y, want) <= 1e-5


def _yaml_model(batch=2, frames=3):
    tool = _tool()
    g = load_golden("mgn_rollout_yaml_delaunay_32x64")
    m, case = _model(g, tool)
    case = dict(case, batch=batch, frames=frames)
    return m, _inputs(tool, "yaml_delaunay_32x64", case)


@pytest.mark.gpu
def test_repeated_rollout_is_bit_identical():
    m, (c, p, q) = _yaml_model()
    a = m(constants=c, prescribed=p, prognostic=q)
    b = m(constants=c, prescribed=p, prognostic=q)
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_step_graphs_bit_identical():
    m, (c, p, q) = _yaml_model()
    plain = m(constants=c, prescribed=p, prognostic=q)
    m.set_step_graphs(True)
    graphed = m(constants=c, prescribed=p, prognostic=q)
    torch.cuda.synchronize()
    assert torch.equal(plain, graphed)


@pytest.mark.gpu
def test_supported_shapes_never_call_torch_composition(monkeypatch):
    from dlwp_benchmark_amd import ops

    def boom(*a, **k):
        raise AssertionError("torch composition called on a HIP-supported shape")

    monkeypatch.setattr(ops, "mgn_layer_torch", boom)
    monkeypatch.setattr(ops, "mgn_mlp_torch", boom)
    m, (c, p, q) = _yaml_model()
    m(constants=c, prescribed=p, prognostic=q)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_default_dispatch_by_width(monkeypatch):
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.models import MeshGraphNet
    from dlwp_benchmark_amd.models.mgn import FUSED_MAX_WIDTH

    calls = []
    real = ops.mgn_layer_torch
    monkeypatch.setattr(ops, "mgn_layer_torch", lambda *a, **k: calls.append(1) or real(*a, **k))
    g = dict(height=4, width=8, periodic=True)
    x = torch.randn(1, 4 + 9, 4, 8, device=DEV)
    with torch.no_grad():
        narrow = MeshGraphNet(**dict(YAML_KW, hidden_dim_processor=FUSED_MAX_WIDTH), graph=g).to(DEV).eval()
        narrow.one_step(x)
        assert not calls
        wide = MeshGraphNet(**dict(YAML_KW, hidden_dim_processor=FUSED_MAX_WIDTH + 32), graph=g).to(DEV).eval()
        wide.one_step(x)
        assert calls                                      # the composition above the measured crossover
        calls.clear()
        wide.set_fused_layers("always").one_step(x)
        assert not calls


YAML_KW = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, context_size=1, processor_size=2,
               hidden_dim_node_encoder=32, hidden_dim_edge_encoder=32, hidden_dim_node_decoder=32, graph_type="grid_2d")


@pytest.mark.gpu
def test_beyond_envelope_falls_back_and_matches():
    from dlwp_benchmark_amd.models import MeshGraphNet

    kw = dict(constant_channels=1, prognostic_channels=2, context_size=1, processor_size=1, hidden_dim_processor=520,
              hidden_dim_node_encoder=16, hidden_dim_edge_encoder=16, hidden_dim_node_decoder=16, graph_type="grid_2d",
              graph=dict(height=4, width=8, periodic=True))
    m = MeshGraphNet(**kw)
    assert not m.hip_supported()
    torch.manual_seed(0)
    for p in m.parameters():
        with torch.no_grad():
            p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 5.0))
    c, q = torch.randn(1, 1, 1, 4, 8), torch.randn(1, 3, 2, 4, 8)
    ref = MeshGraphNet(**kw).double()
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    with torch.no_grad():
        x = [c[:, 0].double(), q[:, 0].double()]
        s1 = q[:, 0].double() + ref._step_torch(torch.cat(x, 1))
        s2 = s1 + ref._step_torch(torch.cat([c[:, 0].double(), s1], 1))
    want = torch.stack([s1, s2], 1)
    m = m.float().to(DEV).eval()
    got = m(constants=c.to(DEV), prognostic=q.to(DEV))
    assert rel_l2(got, want) <= 1e-5


@pytest.mark.gpu
def test_peak_memory_below_torch_concat_at_yaml_batch32():
    m, _ = _yaml_model()
    b, frames = 32, 2
    gen = torch.Generator().manual_seed(0)
    c = torch.randn(b, 1, 4, 32, 64, generator=gen).to(DEV)
    p = torch.randn(b, frames, 1, 32, 64, generator=gen).to(DEV)
    q = torch.randn(b, frames, 8, 32, 64, generator=gen).to(DEV)
    m(constants=c, prescribed=p, prognostic=q)              # warm-up: workspaces, encoded edge table
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m(constants=c, prescribed=p, prognostic=q)
    torch.cuda.synchronize()
    step_peak = torch.cuda.max_memory_allocated() - base
    concat = b * m.n_edges * 3 * 34 * 4                         # the torch composition's [B E, 3 D] concat alone
    assert step_peak < concat, (step_peak, concat)
