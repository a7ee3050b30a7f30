"""GraphCastNet training on the GPU (csrc/graphcast_bwd.hip through training.gc_mlp / training.gc_layer): each backward
kernel against fp64, both autograd Functions against fp64 autograd of the torch composition on irregular bipartite graphs,
whole-model gradients against the REAL reference class (tests/golden/graphcast_grad_l1_8x16.npz,
graphcast_train_*.npz), no torch fallback, determinism, batch independence, memory, the envelope, the torch-backward
cross-check, an Adam trajectory and in-place edits."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_CASES = ["train_yaml_l3_32x64", "train_mean_hl2_relu_l2_8x16", "train_ctx2_noconst_d40_l1_8x16",
               "train_d512_l1_8x16"]


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_graphcast as t
    finally:
        sys.path.pop(0)
    return t


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / max(float(b.double().norm()), 1e-30))


def _graph(n_src, n_dst, n_edges, seed):
    """an irregular bipartite graph in CSC order by destination; every fifth-ish destination and some sources have no edge"""
    from dlwp_benchmark_amd import ops

    rng = np.random.default_rng(seed)
    dst = rng.integers(0, n_dst, n_edges)
    dst[dst % 5 == 3] = 0
    src = rng.integers(0, n_src, n_edges)
    src[src % 7 == 2] = 1
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    deg = np.bincount(dst, minlength=n_dst)
    row_ptr = np.concatenate([[0], np.cumsum(deg)])
    t = lambda a: torch.from_numpy(a.astype(np.int32)).to(DEV)  # noqa: E731
    g = dict(row_ptr=t(row_ptr), src=t(src), dst=t(dst), deg=t(deg), n_src=n_src, n_dst=n_dst)
    g["src_row_ptr"], g["src_perm"] = ops.mgn_source_csr(g["src"], n_src)
    return g


def _mlp(din, dout, d, hl, act="silu", norm=True, seed=0):
    from dlwp_benchmark_amd.models.graphcast import MeshGraphMLP, get_activation

    torch.manual_seed(seed + din * 7 + dout + hl)
    m = MeshGraphMLP(din, dout, d, hl, get_activation(act), "LayerNorm" if norm else None)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.5).add_(1.0)
            else:
                p.normal_(0, 1.0 / np.sqrt(p.shape[1]))
    return m.model.to(DEV)


# ---- kernels ---------------------------------------------------------------------------------------------------------
def _act64(x, act):
    return torch.relu(x) if act == 1 else torch.nn.functional.silu(x) if act == 2 else x


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,batch,rows", [(37, 53, 1, 45), (130, 200, 2, 301), (512, 512, 3, 1700), (1100, 64, 1, 96),
                                            (24, 512, 4, 20011)])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("dz_cf", [False, True])
def test_weight_grad_dense_and_channels_first_match_fp64(k, n, batch, rows, act, dz_cf):
    from dlwp_benchmark_amd import ops

    torch.manual_seed(k + n + rows)
    a = torch.randn(batch * rows, k, device=DEV)
    dz = torch.randn(batch, n, rows, device=DEV) if dz_cf else torch.randn(batch * rows, n, device=DEV)
    dzr = dz.permute(0, 2, 1).reshape(-1, n) if dz_cf else dz
    want = dzr.double().t() @ _act64(a.double(), act)
    dw, db = ops.gc_weight_grad(dict(a_mode=0, a=a, a_batch_stride=rows * k, lda=k, a_act=act), k, n, batch, rows, dz,
                                dz_cf=dz_cf)
    assert _rel(dw, want) <= 1e-5 and _rel(db, dzr.double().sum(0)) <= 1e-5
    # channels-first A [B, K, rows] (the grid embedder's input)
    acf = a.view(batch, rows, k).permute(0, 2, 1).contiguous()
    dw2, _ = ops.gc_weight_grad(dict(a_mode=1, a=acf, a_batch_stride=k * rows, a_act=act), k, n, batch, rows, dz,
                                dz_cf=dz_cf)
    assert torch.equal(dw, dw2)


@pytest.mark.gpu
def test_weight_grad_shared_table_and_column_block():
    from dlwp_benchmark_amd import ops

    torch.manual_seed(1)
    k, n, batch, rows = 70, 96, 3, 515
    a = torch.randn(rows, k, device=DEV)
    dz = torch.randn(batch * rows, n, device=DEV)
    full = torch.zeros(n, 3 * k + 5, device=DEV)
    ops.gc_weight_grad(dict(a_mode=0, a=a, a_batch_stride=0, lda=k), k, n, batch, rows, dz, dw=full[:, k:2 * k], bias=False)
    want = dz.double().view(batch, rows, n).sum(0).t() @ a.double()
    assert _rel(full[:, k:2 * k], want) <= 1e-5
    assert float(full[:, :k].abs().sum()) == 0 and float(full[:, 2 * k:].abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("d", [24, 130, 512])
def test_weight_grad_aggregate_mode_matches_fp64(mean, d):
    from dlwp_benchmark_amd import ops

    g = _graph(40, 333, 1500, d)
    batch, n = 2, 72
    ne = g["src"].numel()
    e = torch.randn(batch * ne, d, device=DEV)
    x = torch.randn(batch * 333, d, device=DEV)
    dz = torch.randn(batch * 333, n, device=DEV)
    dst = g["dst"].long()
    agg = torch.zeros(batch, 333, d, dtype=torch.float64, device=DEV)
    agg.index_add_(1, dst, e.view(batch, ne, d).double())
    if mean:
        agg = agg / g["deg"].clamp(min=1).double().view(1, -1, 1)
    a = torch.cat([agg.reshape(-1, d), x.double()], 1)
    dw, db = ops.gc_weight_grad(dict(a_mode=2, a=x, a_batch_stride=333 * d, lda=d, agg_e=e, agg_batch_stride=ne * d,
                                     agg_width=d, row_ptr=g["row_ptr"], agg_mean=mean), 2 * d, n, batch, 333, dz)
    assert _rel(dw, dz.double().t() @ a) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("d", [24, 64, 200, 512])
@pytest.mark.parametrize("gather", [None, "sum", "mean"])
def test_layernorm_backward_matches_fp64(d, gather):
    from dlwp_benchmark_amd import ops

    torch.manual_seed(d)
    g = _graph(50, 61, 777, d)
    batch, rows = 2, g["src"].numel()
    ln = torch.nn.LayerNorm(d).to(DEV)
    with torch.no_grad():
        ln.weight.normal_(1, 0.3)
        ln.bias.normal_(0, 0.3)
    z = (torch.randn(batch * rows, d, device=DEV) * 2 + 0.5)
    gy = torch.randn(batch * rows, d, device=DEV)
    gagg = torch.randn(batch * 61, d, device=DEV)
    tot = gy.double()
    kw = {}
    if gather:
        idx = g["dst"].long()
        ga = gagg.double().view(batch, 61, d)[:, idx]
        if gather == "mean":
            ga = ga / g["deg"].double()[idx].view(1, -1, 1)
        tot = tot + ga.reshape(-1, d)
        kw = dict(g_agg=gagg, g_agg_bs=61 * d, idx=g["dst"], deg=g["deg"] if gather == "mean" else None)
    z64 = z.double().requires_grad_(True)
    w64, b64 = ln.weight.double().detach().requires_grad_(True), ln.bias.double().detach().requires_grad_(True)
    y = torch.nn.functional.layer_norm(z64, (d,), w64, b64, ln.eps)
    gz_w, gw_w, gb_w = torch.autograd.grad(y, [z64, w64, b64], tot)
    gt, gz, gw, gb = ops.gc_layernorm_backward(z, ln, batch, rows, gy, want_total=True, **kw)
    assert _rel(gt, tot) <= 1e-6
    assert _rel(gz, gz_w) <= 1e-5 and _rel(gw, gw_w) <= 1e-5 and _rel(gb, gb_w) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("batch_sum", [False, True])
def test_segment_sum_orders_and_empty_segments(batch_sum):
    from dlwp_benchmark_amd import ops

    g = _graph(90, 70, 600, 3)
    batch, d = 3, 40
    ne = g["src"].numel()
    x = torch.randn(batch * ne, d, device=DEV)
    xv = x.double().view(batch, ne, d)
    for row_ptr, perm, idx, n in ((g["row_ptr"], None, g["dst"], 70), (g["src_row_ptr"], g["src_perm"], g["src"], 90)):
        want = torch.zeros(batch, n, d, dtype=torch.float64, device=DEV).index_add_(1, idx.long(), xv)
        if batch_sum:
            want = want.sum(0, keepdim=True)
        got = ops.gc_segment_sum(x, batch, row_ptr, perm, n, batch_sum=batch_sum)
        assert _rel(got, want.reshape(-1, d)) <= 1e-6
        empty = torch.bincount(idx.long(), minlength=n) == 0
        assert bool(empty.any()) and float(got.view(-1, n, d)[:, empty].abs().sum()) == 0
    tot = ops.gc_segment_sum(x, batch, None, None, ne, batch_sum=True)
    assert _rel(tot, xv.sum(0)) <= 1e-6


# ---- autograd Functions -----------------------------------------------------------------------------------------------
def _grads64(seqs, fn, inputs, gouts):
    """fp64 autograd of fn(seqs64, inputs64) -> outputs; returns (input grads, [param grads per seq])"""
    s64 = [copy.deepcopy(s).double() for s in seqs]
    ins = [t.detach().double().requires_grad_(True) for t in inputs]
    outs = fn(s64, ins)
    ps = [p for s in s64 for p in s.parameters()]
    gs = torch.autograd.grad(outs, ins + ps, [g.double() for g in gouts], allow_unused=True)
    return gs[:len(ins)], gs[len(ins):]


@pytest.mark.gpu
@pytest.mark.parametrize("hl", [1, 2, 4])
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("kind", ["rows_ln_res", "cf_in", "cf_out_noln", "shared"])
def test_mlp_function_matches_fp64_autograd(hl, act, kind):
    from dlwp_benchmark_amd import ops, training

    batch, rows, din, d = 2, 301, 19 if kind == "cf_in" else 48, 48
    dout = 5 if kind == "cf_out_noln" else d
    seq = _mlp(din, dout, d, hl, act, norm=kind != "cf_out_noln")
    pk = ops.GcMlpWeights()
    if kind == "cf_in":
        x = torch.randn(batch, din, 7, 43, device=DEV, requires_grad=True)
        y = training.gc_mlp(seq, pk, x, batch, rows, mode=1)
    elif kind == "shared":
        x = torch.randn(rows, din, device=DEV)
        y = training.gc_mlp(seq, pk, x, batch, rows, x_bs=0)
    else:
        x = torch.randn(batch * rows, din, device=DEV, requires_grad=True)
        y = training.gc_mlp(seq, pk, x, batch, rows, residual=kind == "rows_ln_res", out_cf=kind == "cf_out_noln")
    gy = torch.randn_like(y)
    y.backward(gy)

    def fn(s64, ins):
        return training.gc_mlp_torch(s64[0], ins[0], batch, rows, 1 if kind == "cf_in" else 0,
                                     0 if kind == "shared" else 1, kind == "rows_ln_res", kind == "cf_out_noln")

    (gx,), gp = _grads64([seq], fn, [x], [gy])
    for p, w in zip(seq.parameters(), gp):
        assert _rel(p.grad, w) <= 1e-5, kind
    if x.requires_grad:
        assert _rel(x.grad, gx) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("agg", ["sum", "mean"])
@pytest.mark.parametrize("hl,act", [(1, "silu"), (2, "relu"), (4, "silu")])
@pytest.mark.parametrize("layout", ["processor_shared_e", "encoder_shared_dst", "decoder"])
def test_layer_function_matches_fp64_autograd(agg, hl, act, layout):
    from dlwp_benchmark_amd import ops, training

    d, batch = 40, 3
    n_src, n_dst = (57, 57) if layout == "processor_shared_e" else (230, 57) if layout == "encoder_shared_dst" else (57, 230)
    g = _graph(n_src, n_dst, 900, hl)
    ne = g["src"].numel()
    es, ns = _mlp(3 * d, d, d, hl, act, seed=1), _mlp(2 * d, d, d, hl, act, seed=2)
    residual = layout == "processor_shared_e"
    e = torch.randn(ne, d, device=DEV, requires_grad=True)                       # one table for the batch
    xs = torch.randn(batch * n_src, d, device=DEV, requires_grad=True)
    if layout == "processor_shared_e":
        xd = xs
    elif layout == "encoder_shared_dst":
        xd = torch.randn(n_dst, d, device=DEV, requires_grad=True)
    else:
        xd = torch.randn(batch * n_dst, d, device=DEV, requires_grad=True)
    x_new, e_new = training.gc_layer(es, ops.GcMlpWeights(split=(d, d, d)), ns, ops.GcMlpWeights(), agg, g, batch, e, xs,
                                     xd, residual)
    gx, ge = torch.randn_like(x_new), torch.randn_like(e_new)
    outs, gouts = ([x_new, e_new], [gx, ge]) if residual else ([x_new], [gx])
    torch.autograd.backward(outs, gouts)
    ins = [e, xs] if xd is xs else [e, xs, xd]

    def fn(s64, t):
        xo, eo = training.gc_layer_torch(s64[0], s64[1], agg, g, batch, t[0], t[1], t[1] if xd is xs else t[2], residual)
        return [xo, eo] if residual else [xo]

    gin, gp = _grads64([es, ns], fn, ins, gouts)
    for t, w in zip(ins, gin):
        assert _rel(t.grad, w) <= 1e-5, layout
    for p, w in zip(list(es.parameters()) + list(ns.parameters()), gp):
        assert _rel(p.grad, w) <= 1e-5, layout


# ---- the model -------------------------------------------------------------------------------------------------------
def _model(tag):
    from dlwp_benchmark_amd.models import GraphCastNet

    tool = _tool()
    g = load_golden(f"graphcast_{tag}")
    case = json.loads(str(g["case"]))
    m = GraphCastNet(f"icospheres_l{case['level']}.json", **case["kwargs"])
    assert tool.mgn_golden.fill(m) == str(g["sha"])
    m.invalidate_packed()
    m = m.to(DEV).train().set_hip_training(True)
    tag_in = tag
    inputs = [t.to(DEV) if t is not None else None for t in tool.case_inputs(tag_in, case["kwargs"], case["frames"])]
    return m, case, g, tool, inputs


def _loss(m, case, inputs):
    c, p, q = inputs
    y = m(constants=c, prescribed=p, prognostic=q)
    return torch.mean((y - q[:, case["kwargs"]["context_size"]:]) ** 2)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["grad_l1_8x16"] + TRAIN_CASES)
def test_model_gradients_match_reference_golden_on_hip_path(tag, monkeypatch):
    m, case, g, tool, inputs = _model(tag)
    assert m.uses_hip_training()
    monkeypatch.setattr(m, "_step_torch", lambda *a: (_ for _ in ()).throw(AssertionError("torch step")))
    loss = _loss(m, case, inputs)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    names = json.loads(str(g["names"]))
    params = dict(m.named_parameters())
    for name, norm, proj in zip(names, g["norms"], g["projs"]):
        grad = params[name].grad.double().cpu()
        got = float(grad.norm())
        assert abs(got - norm) <= 1e-4 * norm + 1e-9, f"{tag} {name}: |grad| {got} vs {norm}"
        probe = tool.W.normal(f"golden/graphcast/{tag}/probe/{name}", tuple(grad.shape), 1.0).double()
        assert abs(float((grad * probe).sum()) - proj) <= 1e-4 * norm * float(probe.norm()) + 1e-9, f"{tag} {name}"


def _yaml(batch=1, frames=None):
    m, case, _, tool, (c, p, q) = _model("train_yaml_l3_32x64")
    if frames is not None:
        q = q[:, :frames].contiguous()
        p = p[:, :frames].contiguous() if p is not None else None
    if batch > 1:
        q = torch.cat([q] + [q + 0.1 * k for k in range(1, batch)])
        c = c.repeat(batch, 1, 1, 1, 1) if c is not None else None
        p = p.repeat(batch, 1, 1, 1, 1) if p is not None else None
    return m, case, (c, p, q)


def _grads(m, case, inputs):
    m.zero_grad(set_to_none=True)
    _loss(m, case, inputs).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.gpu
def test_training_step_launches_no_torch_gemm_or_index_add(monkeypatch):
    from torch.profiler import ProfilerActivity, profile

    m, case, inputs = _yaml()
    monkeypatch.setattr(m, "_step_torch", lambda *a: (_ for _ in ()).throw(AssertionError("torch step")))
    _grads(m, case, inputs)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _grads(m, case, inputs)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if any(s in n.lower() for s in ("gemm", "cijk", "aten::mm", "aten::addmm", "aten::linear",
                                                              "aten::bmm", "aten::matmul", "index_add"))]
    assert not bad, bad
    assert any("weight_grad_kernel" in n for n in names) and any("layernorm_bwd_kernel" in n for n in names), names


@pytest.mark.gpu
def test_gradients_bitwise_reproducible_and_batch_independent():
    m, case, (c, p, q) = _yaml(4)
    a = _grads(m, case, (c, p, q))
    b = _grads(m, case, (c, p, q))
    assert all(torch.equal(a[n], b[n]) for n in a)
    singles = [_grads(m, case, tuple(t[k:k + 1] if t is not None else None for t in (c, p, q))) for k in range(4)]
    for n in a:
        # the loss is a mean over the batch: the B = 4 gradient is the mean of the single-sample ones
        want = sum(s[n] for s in singles) / 4
        assert _rel(a[n], want) <= 1e-5, n
    # each sample's input gradient does not depend on its neighbours
    q1 = q.clone().requires_grad_(True)
    torch.mean(m(constants=c, prescribed=p, prognostic=q1) ** 2).backward()
    q2 = q.clone()
    q2[1:] = q2[1:] * 1.5 + 0.3
    q2.requires_grad_(True)
    torch.mean(m(constants=c, prescribed=p, prognostic=q2) ** 2).backward()
    assert torch.equal(q1.grad[0], q2.grad[0])


@pytest.mark.gpu
def test_peak_memory_at_yaml_width_below_composition():
    m, case, inputs = _yaml(2, frames=3)
    peaks = []
    for hip in (True, False):
        m.set_hip_training(hip)
        _grads(m, case, inputs)
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=False)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = _loss(m, case, inputs)
        loss.backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
    ratio = peaks[0] / peaks[1]
    print(f"graphcast training peak: hip {peaks[0] / 2**20:.1f} MiB, composition {peaks[1] / 2**20:.1f} MiB, ratio {ratio:.3f}")
    assert ratio <= 0.6, (peaks, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(activation_fn="gelu"), dict(hidden_dim=520)])
def test_outside_envelope_trains_on_composition(kw):
    from dlwp_benchmark_amd.models import GraphCastNet

    tool = _tool()
    args = tool._small(**kw)
    m = GraphCastNet("icospheres_l1.json", **args).to(DEV).train().set_hip_training(True)
    assert not m.uses_hip_training()
    c, p, q = [t.to(DEV) if t is not None else None for t in tool.case_inputs("grad_l1_8x16", args, 3)]
    called = []
    orig = m._step_torch
    m._step_torch = lambda x: called.append(1) or orig(x)
    loss = torch.mean((m(constants=c, prescribed=p, prognostic=q) - q[:, 1:]) ** 2)
    loss.backward()
    assert called
    ref = copy.deepcopy(m)
    ref._step_torch = orig.__func__.__get__(ref)
    loss2 = torch.mean((ref(constants=c, prescribed=p, prognostic=q) - q[:, 1:]) ** 2)
    loss2.backward()
    for (n, a), b in zip(m.named_parameters(), ref.parameters()):
        assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-7), n


@pytest.mark.gpu
def test_torch_backward_cross_check_agrees(monkeypatch):
    m, case, _, _, inputs = _model("train_ctx2_noconst_d40_l1_8x16")
    a = _grads(m, case, inputs)
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    b = _grads(m, case, inputs)
    # fp32 autograd of the composition (atomic index_add) loses digits where a weight gradient sums many cancelling
    # edge terms (on the ReLU / mean case the m2g embedder's first weight differs by ~1e-2, the whole gradient by 2e-4;
    # the HIP gradients meet the reference fixtures there); on this SiLU / sum case the whole gradient agrees to 1e-5
    flat = [torch.cat([g[n].flatten() for n in a]) for g in (a, b)]
    assert _rel(flat[0], flat[1]) <= 1e-5
    for n in a:
        assert _rel(a[n], b[n]) <= 2e-2, n


@pytest.mark.gpu
def test_three_adam_steps_match_composition():
    m, case, _, _, inputs = _model("train_ctx2_noconst_d40_l1_8x16")
    ref = copy.deepcopy(m).set_hip_training(False)
    assert m.uses_hip_training() and not ref.uses_hip_training()
    opts = [torch.optim.Adam(x.parameters(), lr=1e-3) for x in (m, ref)]
    for _ in range(3):
        for x, o in zip((m, ref), opts):
            o.zero_grad()
            _loss(x, case, inputs).backward()
            o.step()
    for (n, a), b in zip(m.named_parameters(), ref.parameters()):
        assert _rel(a.detach(), b.detach()) <= 1e-5, n


@pytest.mark.gpu
def test_in_place_parameter_edit_before_backward_raises():
    m, case, _, _, inputs = _model("grad_l1_8x16")
    loss = _loss(m, case, inputs)
    with torch.no_grad():
        m.processor.processor_layers[0].edge_mlp.model[0].weight.mul_(1.01)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
