"""Training through the diffusion U-Net's AttentionBlock on the GPU (AttentionBlock.forward with gradients: the HIP global
attention forward and backward between the block's Linears): gradients of the block and of one diffusion training step of the attention=True
networks against the REAL reference classes (tests/golden/diffattn_grad_*.npz, tools/make_golden_diffusion_attention_grad.py)
at the project's training tolerance, the DLWP_TRAIN_TORCH_BACKWARD=1 cross-check, and the memory bound of a training step."""
import json
import os
import sys

import pytest
import torch

from helpers import load_golden, rel_l2

DEV = "cuda:0"
OPS = ["c8", "c32", "c1024", "c48_dk16"]
NETS = ["diffmunet_h32_64", "diffmunethpx_h32_64"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_diffusion_attention_grad as tool
    finally:
        sys.path.pop(0)
    return tool


def _inputs(g):
    from dlwp_benchmark_amd.weights import normal

    return {a: normal(n, tuple(s), 1.0) for a, n, s in json.loads(str(g["inputs"]))}


def _with_aliases(model, sd):
    """named_parameters() lists a shared module once; the state dict names it under every path"""
    names = {id(p): k for k, p in model.named_parameters()}
    full = {}
    for k, v in model.state_dict(keep_vars=True).items():
        full[k] = sd[names[id(v)]] if id(v) in names else v.detach().clone()
    return full


def _worst_grad_deviation(g, params, probe):
    worst = 0.0
    for i, pname in enumerate(json.loads(str(g["names"]))):
        assert pname in params and params[pname].grad is not None, f"no gradient for {pname}"
        gr = params[pname].grad.detach().double().cpu()
        n_ref, p_ref = float(g["norms"][i]), float(g["projs"][i])
        scale = max(n_ref, 1e-12)
        worst = max(worst, abs(float(gr.norm()) - n_ref) / scale)
        r = probe(pname, gr.shape).double()
        worst = max(worst, abs(float((gr * r).sum()) - p_ref) / (scale * float(r.norm())))
    for key in g.files:
        if key.startswith("grad::"):
            want = torch.from_numpy(g[key]).double()
            got = params[key[6:]].grad.detach().double().cpu()
            worst = max(worst, float((got - want).norm() / want.norm().clamp_min(1e-30)))
    return worst


def _block_step(tag):
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_by_spec

    g = load_golden(f"diffattn_grad_op_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    assert sha == str(g["sha"])
    m = AttentionBlock(**json.loads(str(g["kwargs"])))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    ins = _inputs(g)
    x = ins["x"].to(DEV).requires_grad_(True)
    loss = torch.nn.functional.mse_loss(m(x), ins["target"].to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return g, m, x, loss


@pytest.mark.gpu
@pytest.mark.parametrize("tag", OPS)
def test_block_gradients_match_reference_golden(tag):
    tool = _tool()
    g, m, x, loss = _block_step(tag)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    err_x = rel_l2(x.grad, torch.from_numpy(g["grad_x"]))
    worst = _worst_grad_deviation(g, dict(m.named_parameters()), lambda n, s: tool.grad_probe(tag, n, s))
    print(tag, "dx rel L2 %.2e, worst parameter gradient deviation %.2e" % (err_x, worst))
    assert err_x <= 1e-4 and worst <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("tag", OPS)
def test_block_gradients_match_torch_backward(tag, monkeypatch):
    """the HIP training path against DLWP_TRAIN_TORCH_BACKWARD=1 (torch recomputation of the attention)"""
    _, m, x, loss = _block_step(tag)
    hip = {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in m.named_parameters()}}
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    _, m2, x2, loss2 = _block_step(tag)
    ref = {"x": x2.grad, **{k: p.grad for k, p in m2.named_parameters()}}
    errs = {k: rel_l2(hip[k], ref[k]) for k in hip}
    assert max(errs.values()) <= 2e-5, errs
    assert abs(loss.item() - loss2.item()) <= 2e-5 * abs(loss2.item())


@pytest.mark.gpu
def test_block_training_uses_the_hip_backward(monkeypatch):
    """the block's backward reaches dlwp_global_attn_bwd_f32: with the op broken the step raises"""
    from dlwp_benchmark_amd import lib, ops

    def broken(*a, **k):
        raise lib.DlwpError("dlwp_global_attn_bwd_f32 failed with status -3: test")

    monkeypatch.setattr(ops, "global_attention_backward", broken)
    with pytest.raises(lib.DlwpError, match="status -3"):
        _block_step("c32")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", NETS)
def test_network_training_step_matches_reference_golden(tag):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec

    tool = _tool()
    g = load_golden(f"diffattn_grad_net_{tag}")
    case = json.loads(str(g["kwargs"]))
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=0.7)
    assert sha == str(g["sha"])
    model = getattr(M, case["cls"])(**case["kwargs"])
    model.load_state_dict(_with_aliases(model, sd), strict=True)
    model = model.to(DEV).train()
    args = {k: v.to(DEV) for k, v in _inputs(g).items()}
    loss = tool.train_step_loss(model, args, case)
    loss.backward()
    torch.cuda.synchronize()
    dl = abs(loss.item() - float(g["loss"])) / abs(float(g["loss"]))
    worst = _worst_grad_deviation(g, dict(model.named_parameters()), lambda n, s: tool.grad_probe(tag, n, s))
    print(tag, "loss deviation %.2e, worst gradient deviation %.2e" % (dl, worst))
    assert dl <= 1e-4 and worst <= 1e-4


@pytest.mark.gpu
def test_block_training_allocates_no_n_by_n_tensor():
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_state_dict, normal

    bt, c, h, w = 24, 64, 64, 64                  # N = 4096, d = 64, 4 heads
    m = AttentionBlock(c)
    fill_state_dict(m)
    m = m.to(DEV).train()
    x = normal("gpu/gattn_train/mem", (bt, c, h, w), 1.0).to(DEV).requires_grad_(True)
    gy = normal("gpu/gattn_train/mem_gy", (bt, c, h, w), 1.0).to(DEV)
    m(x).backward(gy)                              # packed weights, .grad tensors, allocator warm
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m(x).backward(gy)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    n, heads, d = h * w, 4, c
    qkv, res, tok = bt * n * heads * 3 * d, bt * n * heads * d, bt * n * c
    bound = 4 * (3 * qkv + 3 * res + 6 * tok + 2 * bt * heads * n) + 64 * 2 ** 20
    print("peak extra %.0f MiB, bound %.0f MiB" % (extra / 2 ** 20, bound / 2 ** 20))
    assert extra < bound, f"peak extra {extra / 2 ** 20:.0f} MiB >= {bound / 2 ** 20:.0f} MiB"
    assert extra < 4 * bt * heads * n * n // 4     # far below one N x N score tensor
