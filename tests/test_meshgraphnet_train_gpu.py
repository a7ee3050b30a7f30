"""MeshGraphNet training on the HIP backward kernels (csrc/mgn_bwd.hip through training.mgn_layer / training.mgn_mlp):
the processor-layer and MLP backwards against fp64 autograd of the torch composition on irregular graphs, whole-model
gradients of multi-step training rollouts against the REAL reference class (tests/golden/mgn_train_*.npz,
tools/make_golden_meshgraphnet.py), no composition on supported shapes, bitwise reproducibility and batch independence,
the memory bound, the composition beyond the envelope, and an Adam trajectory against the composition."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_CASES = ["mean_mp2_grid_8x16", "stencil8_8x16", "ctx2_prescribed_grid_8x16", "grid_nonperiodic_8x16",
               "d48_delaunay_8x16", "d64_delaunay_8x16"]
YAML = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, input_dim_edges=2, context_size=1,
            processor_size=4, hidden_dim_processor=34, hidden_dim_node_encoder=32, hidden_dim_edge_encoder=32,
            hidden_dim_node_decoder=32, graph_type="delaunay")


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_meshgraphnet as t
    finally:
        sys.path.pop(0)
    return t


def _rel(a, b) -> float:
    """rel L2 against the fp64 reference; a reference norm below 1e-6 (every gradient here is O(1) unless it is zero in
    exact arithmetic, e.g. through a LayerNorm of width 1, where fp64 autograd leaves ~1e-13 of roundoff) counts as zero"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    nb = float(torch.linalg.vector_norm(b))
    na = float(torch.linalg.vector_norm(a - b))
    return na / max(nb, 1e-6)


def _random_graph(n, seed):
    """CSC by destination: isolated nodes, in-degree 0..12, repeated sources"""
    gen = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 13, (n,), generator=gen)
    deg[::7] = 0
    src = torch.randint(0, n, (int(deg.sum()),), generator=gen)
    src[1::5] = src[0::5][:src[1::5].numel()]             # repeated sources
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).int()
    dst = torch.repeat_interleave(torch.arange(n), deg).int()
    return row_ptr, src.int(), dst, deg.int()


def _init(*mlps):
    for m in mlps:
        for p in m.parameters():
            with torch.no_grad():
                p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 5.0))
        with torch.no_grad():
            if isinstance(m.model[-1], torch.nn.LayerNorm):
                m.model[-1].weight.add_(1.0)


# (D, Linears, aggregation, shared edge table, batch, de_out present)
LAYER_CASES = [(1, 2, "sum", True, 1, False), (8, 3, "mean", False, 3, True), (34, 2, "sum", True, 3, True),
               (34, 5, "mean", True, 1, False), (48, 4, "sum", False, 1, True), (48, 2, "mean", True, 3, False),
               (64, 3, "sum", False, 3, False), (64, 2, "mean", True, 3, True), (8, 5, "sum", False, 1, True),
               (64, 5, "mean", False, 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,lins,agg,shared,b,with_de", LAYER_CASES)
def test_processor_layer_backward_matches_fp64(dim, lins, agg, shared, b, with_de):
    _check_layer(dim, lins, agg, shared, b, with_de, 97)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [34, 64])          # parameter partials in LDS (34) and in the global partial row (64)
def test_processor_layer_backward_many_tiles_matches_fp64(dim):
    """3 x 12000 destination nodes: at least 563 tiles of at most 64 nodes, more than the 512 partial-writing
    workgroups, so workgroups loop over several tiles and accumulate their partials across them.  At 216k edges some
    ReLU pre-activations lie within fp32 rounding of 0, so ANY fp32 evaluation flips their masks: the fp32 composition
    itself is ~5e-4 off fp64 on this instance (2e-7 on the 97-node graphs).  The bound is therefore twice the fp32
    composition's own error per tensor, at least 1e-5."""
    _check_layer(dim, 3, "sum", True, 3, True, 12000, calibrate=True)


def _check_layer(dim, lins, agg, shared, b, with_de, n, calibrate=False):
    from dlwp_benchmark_amd import ops, training
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    torch.manual_seed(dim * 100 + lins)
    row_ptr, src, dst, deg = _random_graph(n, dim + lins)
    ne = src.numel()
    em, nm = MeshGraphMLP(3 * dim, dim, dim, lins - 1), MeshGraphMLP(2 * dim, dim, dim, lins - 1)
    _init(em, nm)
    x = torch.randn(b * n, dim)
    e = torch.randn(ne if shared else b * ne, dim)
    gx, ge = torch.randn(b * n, dim), torch.randn(b * ne, dim)
    # fp64 reference
    em64, nm64 = MeshGraphMLP(3 * dim, dim, dim, lins - 1).double(), MeshGraphMLP(2 * dim, dim, dim, lins - 1).double()
    em64.load_state_dict(em.state_dict()), nm64.load_state_dict(nm.state_dict())
    x64, e64 = x.double().requires_grad_(True), e.double().requires_grad_(True)
    xo, eo = ops.mgn_layer_torch(em64.model, nm64.model, agg, src, dst, deg, b, x64, e64)
    loss = (xo * gx.double()).sum() + ((eo * ge.double()).sum() if with_de else 0.0)
    loss.backward()
    tol = {}
    if calibrate:                                       # the fp32 composition's own error on this instance
        em32, nm32 = MeshGraphMLP(3 * dim, dim, dim, lins - 1), MeshGraphMLP(2 * dim, dim, dim, lins - 1)
        em32.load_state_dict(em.state_dict()), nm32.load_state_dict(nm.state_dict())
        x32, e32 = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
        xo32, eo32 = ops.mgn_layer_torch(em32.model, nm32.model, agg, src, dst, deg, b, x32, e32)
        ((xo32 * gx).sum() + ((eo32 * ge).sum() if with_de else 0.0)).backward()
        tol["dx"], tol["de"] = _rel(x32.grad, x64.grad), _rel(e32.grad, e64.grad)
        for i, (p32, p64) in enumerate(zip(list(em32.parameters()) + list(nm32.parameters()),
                                           list(em64.parameters()) + list(nm64.parameters()))):
            tol[i] = _rel(p32.grad, p64.grad)
    tol = {k: max(1e-5, 2 * v) for k, v in tol.items()}
    # HIP
    emd, nmd = em.to(DEV), nm.to(DEV)
    csr = ops.mgn_source_csr(src.to(DEV), n)
    graph = (row_ptr.to(DEV), src.to(DEV), dst.to(DEV), deg.to(DEV), *csr)
    xd, ed = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    xo_d, eo_d = training.mgn_layer(emd.model, ops.MgnMlpWeights(), nmd.model, ops.MgnMlpWeights(), agg, graph, b, xd, ed,
                                    shared)
    loss_d = (xo_d * gx.to(DEV)).sum() + ((eo_d * ge.to(DEV)).sum() if with_de else 0.0)
    loss_d.backward()
    torch.cuda.synchronize()
    case = (dim, lins, agg, shared, b, with_de)
    assert _rel(xo_d, xo) <= 1e-5, case
    assert _rel(xd.grad, x64.grad) <= tol.get("dx", 1e-5), (case, "dx", _rel(xd.grad, x64.grad), tol.get("dx"))
    assert _rel(ed.grad, e64.grad) <= tol.get("de", 1e-5), (case, "de", _rel(ed.grad, e64.grad), tol.get("de"))
    for i, ((name, p), p64) in enumerate(zip(list(emd.named_parameters()) + list(nmd.named_parameters()),
                                             list(em64.parameters()) + list(nm64.parameters()))):
        assert _rel(p.grad, p64.grad) <= tol.get(i, 1e-5), (case, i, name, _rel(p.grad, p64.grad), tol.get(i))


# (input width, hidden, output, Linears, LayerNorm)
MLP_CASES = [(256, 64, 64, 2, True), (256, 64, 64, 3, False), (13, 32, 8, 2, False), (192, 64, 64, 5, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,hid,cout,lins,norm", MLP_CASES)
@pytest.mark.parametrize("cf_in,cf_out", [(False, False), (True, False), (False, True), (True, True)])
def test_mlp_backward_matches_fp64(cin, hid, cout, lins, norm, cf_in, cf_out):
    _check_mlp(cin, hid, cout, lins, norm, cf_in, cf_out, 77)          # 231 rows: tiles straddle the samples


@pytest.mark.gpu
def test_mlp_backward_many_tiles_matches_fp64():
    """3 x 20000 rows: at least 938 tiles of at most 64 rows, more than the 512 partial-writing workgroups"""
    _check_mlp(13, 32, 34, 2, True, True, False, 20000)


def _check_mlp(cin, hid, cout, lins, norm, cf_in, cf_out, rows):
    from dlwp_benchmark_amd import ops, training
    from dlwp_benchmark_amd.models.mgn import MeshGraphMLP

    torch.manual_seed(cin + hid + lins)
    b = 3
    m = MeshGraphMLP(cin, cout, hid, lins - 1, norm=norm)
    _init(m)
    x = torch.randn(b, cin, rows) if cf_in else torch.randn(b * rows, cin)
    g = torch.randn(b, cout, rows) if cf_out else torch.randn(b * rows, cout)
    m64 = MeshGraphMLP(cin, cout, hid, lins - 1, norm=norm).double()
    m64.load_state_dict(m.state_dict())
    x64 = x.double().requires_grad_(True)
    y64 = m64.model(training._mgn_rows(x64, b, rows, cf_in))
    if cf_out:
        y64 = y64.view(b, rows, cout).permute(0, 2, 1)
    (y64 * g.double()).sum().backward()
    md = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = training.mgn_mlp(md.model, ops.MgnMlpWeights(), xd, b, rows, cf_in, cf_out)
    (y * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert y.shape == y64.shape
    assert _rel(y, y64) <= 1e-5
    assert _rel(xd.grad, x64.grad) <= 1e-5, _rel(xd.grad, x64.grad)
    for (name, p), p64 in zip(md.named_parameters(), m64.parameters()):
        assert _rel(p.grad, p64.grad) <= 1e-5, (name, _rel(p.grad, p64.grad))


def _golden_model(g, tool):
    from dlwp_benchmark_amd.models import MeshGraphNet

    case = json.loads(str(g["case"]))
    h, w, periodic = case["graph"]
    m = MeshGraphNet(**case["kwargs"], graph=dict(height=h, width=w, periodic=periodic))
    assert tool.fill(m) == str(g["sha"])
    m.invalidate_packed()
    m.set_fused_layers("always")            # the kernels at every width of the fixtures, 48 and 64 included
    return m.to(DEV).train(), case


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TRAIN_CASES)
def test_training_gradients_match_reference_golden(tag):
    tool = _tool()
    g = load_golden(f"mgn_train_{tag}")
    m, case = _golden_model(g, tool)
    assert m.uses_hip_training()
    c, p, q = (t.to(DEV) if t is not None else None
               for t in tool.case_inputs(tag, case["kwargs"], case["batch"], case["frames"], case["graph"][:2]))
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
        projs.append(float((gr * tool.W.normal(f"golden/mgn/{tag}/probe/{name}", tuple(gr.shape), 1.0).double()).sum()))
    np.testing.assert_allclose(norms, g["norms"], rtol=1e-4, atol=1e-4 * float(np.max(g["norms"])))
    np.testing.assert_allclose(projs, g["projs"], rtol=1e-4, atol=1e-4 * float(np.max(np.abs(g["projs"]))))


def _yaml_model(h, w, seed=0, **kw):
    from dlwp_benchmark_amd.models import MeshGraphNet

    m = MeshGraphNet(**dict(YAML, **kw), graph=dict(height=h, width=w, periodic=True))
    torch.manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 5.0))
        for mod in m.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.add_(1.0)                     # LayerNorm scales around 1
    m.invalidate_packed()
    return m.to(DEV).train()


def _inputs(m, b, h, w, frames, seed=1):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randn(b, 1, YAML["constant_channels"], h, w, generator=gen)
    p = torch.randn(b, frames, YAML["prescribed_channels"], h, w, generator=gen)
    q = torch.randn(b, frames, YAML["prognostic_channels"], h, w, generator=gen)
    return c.to(DEV), p.to(DEV), q.to(DEV)


@pytest.mark.gpu
def test_training_step_runs_no_composition(monkeypatch):
    from dlwp_benchmark_amd import ops

    def boom(*a, **k):
        raise AssertionError("torch composition called in a HIP training step")

    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "0")
    monkeypatch.setattr(ops, "mgn_layer_torch", boom)
    monkeypatch.setattr(ops, "mgn_mlp_torch", boom)
    m = _yaml_model(8, 16)
    c, p, q = _inputs(m, 2, 8, 16, 3)
    y = m(constants=c, prescribed=p, prognostic=q)
    torch.mean((y - q[:, 1:]) ** 2).backward()
    assert all(p_.grad is not None for p_ in m.parameters())


@pytest.mark.gpu
def test_gradients_bitwise_reproducible_and_batch_independent():
    m = _yaml_model(8, 16)
    c, p, q = _inputs(m, 4, 8, 16, 3)

    def grads(c_, p_, q_):
        m.zero_grad(set_to_none=True)
        q_ = q_.clone().requires_grad_(True)
        y = m(constants=c_, prescribed=p_, prognostic=q_)
        ((y - 0.5) ** 2).sum().backward()             # a sum: each sample's input gradient is its own
        torch.cuda.synchronize()
        return q_.grad.clone(), [p_.grad.clone() for p_ in m.parameters()]

    gq1, gp1 = grads(c, p, q)
    gq2, gp2 = grads(c, p, q)
    assert torch.equal(gq1, gq2)
    assert all(torch.equal(a, b) for a, b in zip(gp1, gp2))
    for i in range(4):
        gqi, _ = grads(c[i:i + 1], p[i:i + 1], q[i:i + 1])
        assert torch.equal(gqi[0], gq1[i]), i


@pytest.mark.gpu
def test_training_peak_memory_below_half_of_composition():
    from dlwp_benchmark_amd.rollout import rollout_train

    m = _yaml_model(32, 64)
    assert m.uses_hip_training()
    c, p, q = _inputs(m, 32, 32, 64, 3)

    def peak(fn):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = fn()
        torch.mean((y - q[:, 1:]) ** 2).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    peak(lambda: m(constants=c, prescribed=p, prognostic=q))          # warm-up (packed weights, workspaces)
    hip = peak(lambda: m(constants=c, prescribed=p, prognostic=q))
    comp = peak(lambda: rollout_train(m._step_torch, m.context_size, c, p, q))
    assert hip < 0.5 * comp, (hip / 2 ** 20, comp / 2 ** 20)


def _fp64_reference_grads(m, c, p, q):
    """the composition in fp64 on the CPU: (loss, {name: grad})"""
    import copy

    from dlwp_benchmark_amd.rollout import rollout_train

    m64 = copy.deepcopy(m).cpu().double()
    c64, p64, q64 = (t.detach().cpu().double() for t in (c, p, q))
    y = rollout_train(m64._step_torch, m64.context_size, c64, p64, q64)
    loss = torch.mean((y - q64[:, m64.context_size:]) ** 2)
    loss.backward()
    return float(loss.detach()), {n: p_.grad for n, p_ in m64.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("dim,mode", [(96, "always"), (520, "auto")])
def test_beyond_envelope_trains_on_composition(dim, mode):
    m = _yaml_model(4, 8, hidden_dim_processor=dim, processor_size=2).set_fused_layers(mode)
    assert not m.uses_hip_training()
    c, p, q = _inputs(m, 2, 4, 8, 3)
    y = m(constants=c, prescribed=p, prognostic=q)
    loss = torch.mean((y - q[:, 1:]) ** 2)
    loss.backward()
    want_loss, want = _fp64_reference_grads(m, c, p, q)
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
    for n, p_ in m.named_parameters():          # the fp32 composition's GEMMs (K up to 3D = 1560) against fp64
        assert _rel(p_.grad, want[n]) <= 1e-3, (n, _rel(p_.grad, want[n]))


@pytest.mark.gpu
def test_adam_trajectory_matches_composition():
    from dlwp_benchmark_amd.rollout import rollout_train

    losses = {}
    for path in ("hip", "torch"):
        m = _yaml_model(8, 16, seed=3)
        c, p, q = _inputs(m, 2, 8, 16, 3, seed=4)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = []
        for _ in range(5):
            opt.zero_grad(set_to_none=True)
            if path == "hip":
                y = m(constants=c, prescribed=p, prognostic=q)
            else:
                y = rollout_train(m._step_torch, m.context_size, c, p, q)
            loss = torch.mean((y - q[:, 1:]) ** 2)
            loss.backward()
            opt.step()
            out.append(float(loss))
        losses[path] = out
    np.testing.assert_allclose(losses["hip"], losses["torch"], rtol=1e-4)


@pytest.mark.gpu
def test_in_place_parameter_edit_before_backward_raises():
    """the Functions save their parameters: an in-place edit between forward and backward trips autograd's version
    check, as it does for the composition, instead of differentiating the edited weights"""
    m = _yaml_model(8, 16)
    c, p, q = _inputs(m, 2, 8, 16, 3)
    y = m(constants=c, prescribed=p, prognostic=q)
    with torch.no_grad():
        m.processor.processor_layers[0].edge_mlp.model[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.mean((y - q[:, 1:]) ** 2).backward()
