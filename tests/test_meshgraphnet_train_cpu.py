"""MeshGraphNet training plumbing without a GPU: the source-sorted edge permutation of the backward's source-side gather,
the backward envelope, and DLWP_TRAIN_TORCH_BACKWARD=1 selecting the torch composition in the autograd Functions'
backward (training._MgnLayerFn / _MgnMlpFn)."""
import types

import numpy as np
import pytest
import torch

YAML = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, input_dim_edges=2, context_size=1,
            processor_size=4, hidden_dim_processor=34, hidden_dim_node_encoder=32, hidden_dim_edge_encoder=32,
            hidden_dim_node_decoder=32)


@pytest.mark.parametrize("graph_type,hw,periodic", [("grid_2d", (8, 16), False), ("grid_2d_8stencil", (8, 16), True),
                                                    ("delaunay", (32, 64), True)])
def test_source_permutation_holds_every_edge_once_sorted_by_source(graph_type, hw, periodic):
    from dlwp_benchmark_amd.models import MeshGraphNet

    kw = dict(YAML, graph_type=graph_type, input_dim_edges=3 if graph_type == "grid_2d_8stencil" else 2)
    m = MeshGraphNet(**kw, graph=dict(height=hw[0], width=hw[1], periodic=periodic))
    perm = m.graph_src_perm.long().numpy()
    row_ptr = m.graph_src_row_ptr.long().numpy()
    src = m.graph_src.long().numpy()
    assert np.array_equal(np.sort(perm), np.arange(m.n_edges))                 # every edge exactly once
    assert np.all(np.diff(src[perm]) >= 0)                                     # sorted by source
    for n in range(m.n_nodes):
        seg = perm[row_ptr[n]:row_ptr[n + 1]]
        assert np.all(src[seg] == n)
        assert np.all(np.diff(seg) > 0)                                        # stable: CSC order within a source
    assert row_ptr[0] == 0 and row_ptr[-1] == m.n_edges
    sd = m.state_dict()
    assert not any(k.startswith("graph_") for k in sd)
    assert "graph_src_perm" not in m._buffers or "graph_src_perm" in m._non_persistent_buffers_set
    assert "graph_src_row_ptr" in m._non_persistent_buffers_set


def test_ops_source_csr_matches_model():
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.models import MeshGraphNet

    m = MeshGraphNet(**YAML, graph_type="grid_2d", graph=dict(height=8, width=16, periodic=True))
    rp, perm = ops.mgn_source_csr(m.graph_src, m.n_nodes)
    assert torch.equal(rp, m.graph_src_row_ptr) and torch.equal(perm, m.graph_src_perm)


def test_backward_envelope():
    from dlwp_benchmark_amd.models import MeshGraphNet

    g = dict(height=8, width=16, periodic=True)
    assert MeshGraphNet(**YAML, graph_type="grid_2d", graph=g).uses_hip_training()
    m64 = MeshGraphNet(**dict(YAML, hidden_dim_processor=64), graph_type="grid_2d", graph=g)
    assert not m64.uses_hip_training()                  # measured slower than the composition: TRAIN_FUSED_MAX_WIDTH
    assert m64.set_fused_layers("always").uses_hip_training()
    m96 = MeshGraphNet(**dict(YAML, hidden_dim_processor=96), graph_type="grid_2d", graph=g).set_fused_layers("always")
    assert m96.uses_fused_layers() and not m96.uses_hip_training()
    wide_enc = MeshGraphNet(**dict(YAML, hidden_dim_node_encoder=65), graph_type="grid_2d", graph=g)
    assert not wide_enc.set_fused_layers("always").uses_hip_training()


def _small_layer(dim=6, lins=2):
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    torch.manual_seed(0)
    em, nm = MeshGraphMLP(3 * dim, dim, dim, lins - 1).double(), MeshGraphMLP(2 * dim, dim, dim, lins - 1).double()
    n, b = 9, 2
    deg = torch.tensor([0, 2, 1, 3, 0, 1, 2, 2, 1])
    src = torch.tensor([3, 5, 0, 1, 1, 8, 2, 7, 4, 6, 0, 3]).int()
    dst = torch.repeat_interleave(torch.arange(n), deg).int()
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).int()
    x = torch.randn(b * n, dim, dtype=torch.float64)
    e = torch.randn(src.numel(), dim, dtype=torch.float64)
    return em, nm, (row_ptr, src, dst, deg.int()), b, x, e


def test_torch_backward_env_selects_composition_for_layer(monkeypatch):
    from dlwp_benchmark_amd import ops, training

    em, nm, (row_ptr, src, dst, deg), b, x, e = _small_layer()
    graph = (row_ptr, src, dst, deg, *ops.mgn_source_csr(src, deg.numel()))
    cfg = (em.model, None, nm.model, None, "mean", graph, b)
    dx_out = torch.randn(b * deg.numel(), x.shape[1], dtype=torch.float64)
    de_out = torch.randn(b * src.numel(), x.shape[1], dtype=torch.float64)
    ctx = types.SimpleNamespace(saved_tensors=(x, e), cfg=cfg, e_shared=True, needs_input_grad=(True, True))
    called = []
    monkeypatch.setattr(ops, "mgn_processor_layer_backward", lambda *a, **k: called.append(1) or (_ for _ in ()).throw(
        RuntimeError("HIP backward")))
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    out = training._MgnLayerFn.backward(ctx, dx_out, de_out)
    assert not called
    # against autograd of the composition
    x_, e_ = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    xo, eo = ops.mgn_layer_torch(em.model, nm.model, "mean", src, dst, deg, b, x_, e_)
    params = list(em.parameters()) + list(nm.parameters())
    want = torch.autograd.grad([xo, eo], [x_, e_] + params, [dx_out, de_out])
    assert len(out) == 4 + len(params)
    assert out[2] is None and out[3] is None
    for got, w in zip(out[:2] + out[4:], want):
        torch.testing.assert_close(got, w)
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "0")
    with pytest.raises(RuntimeError, match="HIP backward"):
        training._MgnLayerFn.backward(ctx, dx_out, de_out)
    assert called


def test_torch_backward_env_selects_composition_for_mlp(monkeypatch):
    from dlwp_benchmark_amd import ops, training
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    torch.manual_seed(1)
    m = MeshGraphMLP(5, 3, 4, 2).double()
    b, rows = 2, 7
    x = torch.randn(b, 5, rows, dtype=torch.float64)               # channels-first in
    gy = torch.randn(b * rows, 3, dtype=torch.float64)
    ctx = types.SimpleNamespace(saved_tensors=(x,), cfg=(m.model, None, b, rows, True, False),
                                needs_input_grad=(True,) + (False,) * 6)
    monkeypatch.setattr(ops, "mgn_mlp_backward", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("HIP backward")))
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    out = training._MgnMlpFn.backward(ctx, gy)
    x_ = x.clone().requires_grad_(True)
    y = m.model(x_.permute(0, 2, 1).reshape(b * rows, 5))
    want = torch.autograd.grad(y, [x_] + list(m.parameters()), gy)
    torch.testing.assert_close(out[0], want[0])
    for got, w in zip(out[7:], want[1:]):
        torch.testing.assert_close(got, w)
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "0")
    with pytest.raises(RuntimeError, match="HIP backward"):
        training._MgnMlpFn.backward(ctx, gy)
