"""Training through GroupNorm + activation on the GPU: ops.groupnorm_act under autograd runs dlwp_groupnorm_act_fwd_stats_f32
and dlwp_groupnorm_act_bwd_f32 (csrc/groupnorm_bwd.hip).

Kernel variants and the case of test_groupnorm_bwd_cpu.CASES that reaches each.  The row-sum and the dx kernel come in four
forms, {16-byte loads, 4-byte loads} x {G <= 64 lanes per row with 256 / G rows per workgroup, one row per workgroup}:
  vector, G lanes      rows_of_4 (HW 4: G = 1, all 16 rows in one workgroup, one channel per group: the workgroup derives
                       a, b of 16 (sample, group) pairs, one lane each), one_group (HW 64: G = 16, whole sample one group,
                       16 lanes sum a, b), rows1632 (1632 rows: 102 workgroups, more than one per sample; cpg 136 > 64: the
                       a, b sum wraps its 64 lanes)
  vector, workgroup    rank3_300 (75 loads: lanes 75 .. 255 idle), hw1056 (264 loads: the sweep wraps)
  scalar, G lanes      hw35 (G = 64, 35 lanes busy, 4 rows per workgroup, 36 rows: the last workgroup is part empty),
                       offset_view (HW 16 with 4-byte-aligned x and gy: the launcher must not take the vector form)
  scalar, workgroup    hw257 (added to the issue's list, which has no long row with HW % 4 != 0: the sweep wraps)
The dgamma / dbeta kernel has one form: 8 channels per workgroup (rows1632: 17 workgroups; hw35 12 channels: the second is
half empty), 128 samples per LDS chunk (no case has more than 128 samples: a second chunk is the same loop body).

A gradient that is zero in exact arithmetic (constant output gradient and identity activation: dx without affine or with one
channel per group, dgamma with one channel per group) is measured against the size of its terms instead of against that
zero: see test_groupnorm_bwd_cpu.term_norms."""
import json
import os
import sys

import pytest
import torch

from helpers import load_golden, rel_l2
from test_groupnorm_bwd_cpu import ACT_FNS, CASES, deviation, inputs, reference, term_norms

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = [0, 1, 2, 3, 4]


def _dev(t, offset):
    """t on the GPU, contiguous; offset: as a view that starts one float into its storage (4-byte-aligned pointer)"""
    if t is None:
        return None
    if not offset:
        return t.to(DEV)
    store = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    view = store[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _run(tag, act, affine, mean_gy=False, x_grad=True, wb_grad=True):
    """one forward + backward of ops.groupnorm_act on the GPU: (y, dx, dgamma, dbeta, grad_fn)"""
    from dlwp_benchmark_amd import ops

    _, groups, offset = CASES[tag]
    x, gamma, beta, gy = inputs(tag)
    x = _dev(x, offset).requires_grad_(x_grad)
    gamma = gamma.to(DEV).requires_grad_(wb_grad) if affine else None
    beta = beta.to(DEV).requires_grad_(wb_grad) if affine else None
    y = ops.groupnorm_act(x, gamma, beta, groups, 1e-5, act)
    if mean_gy:
        y.mean().backward()
    else:
        y.backward(_dev(gy, offset))
    torch.cuda.synchronize()
    return y.detach(), x.grad, gamma.grad if affine else None, beta.grad if affine else None, y.grad_fn


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("tag", list(CASES))
def test_op_gradients_match_fp64_autograd(tag, act):
    worst = {}
    for affine in (True, False):
        for mean_gy in (False, True):
            _, dx, dgamma, dbeta, fn = _run(tag, act, affine, mean_gy)
            assert "_GroupNormActFn" in type(fn).__name__, type(fn).__name__
            want = reference(tag, act, affine, mean_gy)
            scale = term_norms(tag, act, affine, mean_gy)
            errs = {"dx": deviation(dx, want[0], scale[0])}
            if affine:
                errs["dgamma"], errs["dbeta"] = deviation(dgamma, want[1], scale[1]), deviation(dbeta, want[2], scale[2])
            print(tag, act, "affine" if affine else "plain", "mean" if mean_gy else "dense",
                  {k: "%.2e" % v for k, v in errs.items()})
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
    assert max(worst.values()) <= 1e-5, worst


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_training_forward_is_bit_equal_to_inference(tag):
    from dlwp_benchmark_amd import ops

    _, groups, offset = CASES[tag]
    x, gamma, beta, _ = inputs(tag)
    x, gamma, beta = _dev(x, offset), gamma.to(DEV), beta.to(DEV)
    for act in ACTS:
        for g, b in ((gamma, beta), (None, None)):
            with torch.no_grad():
                want = ops.groupnorm_act(x, g, b, groups, 1e-5, act)
            xr = x.detach().requires_grad_(True)
            got = ops.groupnorm_act(xr, g, b, groups, 1e-5, act)
            assert got.requires_grad and torch.equal(got.detach(), want), (act, g is not None)
            # and it is GroupNorm: against fp64 on the CPU at the fp32 bound
            ref = ACT_FNS[act](torch.nn.functional.group_norm(x.double().cpu(), groups, g.double().cpu() if g is not None else None,
                                                              b.double().cpu() if b is not None else None, 1e-5))
            assert rel_l2(got, ref) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_backward_reruns_are_bitwise_identical(tag):
    for act in (1, 4):
        first = _run(tag, act, True)[1:4]
        again = _run(tag, act, True)[1:4]
        for a, b in zip(first, again):
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["one_group", "hw35", "rank3_300"])
def test_only_x_statistics_and_affine_are_saved(tag):
    shape, groups, _ = CASES[tag]
    numel = 1
    for s in shape:
        numel *= s
    from dlwp_benchmark_amd import ops

    x, gamma, beta, _ = inputs(tag)
    for affine in (True, False):
        y = ops.groupnorm_act(x.to(DEV).requires_grad_(True), gamma.to(DEV) if affine else None,
                              beta.to(DEV) if affine else None, groups, 1e-5, 1)
        saved = sum(t.numel() for t in y.grad_fn.saved_tensors)
        assert saved == numel + 2 * shape[0] * groups + (2 * shape[1] if affine else 0), (saved, affine)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["one_group", "hw35"])
def test_needs_input_grad_is_honoured(tag, monkeypatch):
    from dlwp_benchmark_amd import ops

    calls = []
    real = ops.groupnorm_act_backward

    def spy(*a, **k):
        calls.append(a[7:10])
        return real(*a, **k)

    monkeypatch.setattr(ops, "groupnorm_act_backward", spy)
    _, dx, dgamma, dbeta, _ = _run(tag, 1, True, x_grad=False)
    want = reference(tag, 1, True)
    assert dx is None and calls[-1] == (False, True, True)
    assert rel_l2(dgamma, want[1]) <= 1e-5 and rel_l2(dbeta, want[2]) <= 1e-5
    _, dx, dgamma, dbeta, _ = _run(tag, 1, False)
    assert dgamma is None and dbeta is None and calls[-1] == (True, False, False)
    assert rel_l2(dx, reference(tag, 1, False)[0]) <= 1e-5
    # x and beta only: no dgamma buffer
    _, groups, _ = CASES[tag]
    x, gamma, beta, gy = inputs(tag)
    x, gamma, beta = x.to(DEV).requires_grad_(True), gamma.to(DEV), beta.to(DEV).requires_grad_(True)
    ops.groupnorm_act(x, gamma, beta, groups, 1e-5, 1).backward(gy.to(DEV))
    assert calls[-1] == (True, False, True) and gamma.grad is None
    assert rel_l2(x.grad, want[0]) <= 1e-5 and rel_l2(beta.grad, want[2]) <= 1e-5


@pytest.mark.gpu
def test_bad_arguments_raise():
    from dlwp_benchmark_amd import lib, ops

    x = torch.zeros(2, 6, 4, 4, device=DEV, requires_grad=True)
    with pytest.raises(lib.DlwpError):
        ops.groupnorm_act(x, None, None, 4, 1e-5, 0)              # 6 channels in 4 groups
    with pytest.raises(lib.DlwpError):
        ops.groupnorm_act(x, None, None, 3, 1e-5, 7)              # no activation 7
    stats = torch.zeros(2, 3, 2, device=DEV)
    with pytest.raises(lib.DlwpError):
        ops.groupnorm_act_backward(x.detach(), stats, None, None, torch.zeros_like(x), 3, 7)
    with pytest.raises(lib.DlwpError):
        ops.groupnorm_act_backward(x.detach(), stats, None, None, torch.zeros_like(x), 4, 0)


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def _hpx_step(tag):
    """tests/test_hpx_train_gpu.py::_step: the fixture's model in train mode, one rollout-MSE backward"""
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.make_golden import hpx_inputs, rollout_mse

    tool = _tool("make_golden_hpx_grad")
    _, cls, base, (cfg, (batch, frames), hw) = tool.NET_CASES[tag]
    g = load_golden(f"grad_hpx_{tag}")
    model = getattr(M, cls)(**cfg)
    assert fill_state_dict(model, gain=1.0) == str(g["sha"]), "filler drifted: regenerate fixtures"
    model = model.to(DEV).train()
    dev = lambda t: t.to(DEV) if t is not None else None
    constants, prescribed, prognostic = [dev(t) for t in hpx_inputs(base, cfg, batch, frames, hw)]
    y = model(constants=constants, prescribed=prescribed, prognostic=prognostic)
    loss = rollout_mse(y, prognostic, cfg["context_size"])
    loss.backward()
    torch.cuda.synchronize()
    return g, model, loss, lambda n, s: tool.grad_probe(tag, n, s)


def _diffusion_step(tag):
    """tests/test_diffusion_attention_train_gpu.py::test_network_training_step_matches_reference_golden's driver"""
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec, normal

    tool = _tool("make_golden_diffusion_attention_grad")
    g = load_golden(f"diffattn_grad_net_{tag}")
    case = json.loads(str(g["kwargs"]))
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=0.7)
    assert sha == str(g["sha"])
    model = getattr(M, case["cls"])(**case["kwargs"])
    names = {id(p): k for k, p in model.named_parameters()}      # a shared module is listed once, the state dict names every path
    full = {k: sd[names[id(v)]] if id(v) in names else v.detach().clone() for k, v in model.state_dict(keep_vars=True).items()}
    model.load_state_dict(full, strict=True)
    model = model.to(DEV).train()
    args = {a: normal(n, tuple(s), 1.0).to(DEV) for a, n, s in json.loads(str(g["inputs"]))}
    loss = tool.train_step_loss(model, args, case)
    loss.backward()
    torch.cuda.synchronize()
    return g, model, loss, lambda n, s: tool.grad_probe(tag, n, s)


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


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["munethpx_h16_8_norm", "diffmunet_h32_64", "diffmunethpx_h32_64"])
def test_networks_train_without_torch_group_norm(net, monkeypatch):
    """the reference classes' gradients (the fixtures of the HEALPix and the diffusion training tests) with torch's GroupNorm
    out of reach: every norm1 / norm2 / final_norm of the step runs the HIP forward and backward"""
    def boom(*a, **k):
        raise AssertionError("the training step left the library for torch.nn.functional.group_norm")

    monkeypatch.setattr(torch.nn.functional, "group_norm", boom)
    g, model, loss, probe = _hpx_step(net) if net.startswith("munethpx") else _diffusion_step(net)
    dl = abs(loss.item() - float(g["loss"])) / abs(float(g["loss"]))
    worst = _worst_grad_deviation(g, dict(model.named_parameters()), probe)
    print(net, "loss deviation %.2e, worst gradient deviation %.2e" % (dl, worst))
    assert dl <= 1e-5 and worst <= 1e-4


@pytest.mark.gpu
def test_torch_backward_switch_agrees_with_hip(monkeypatch):
    _, hip, _, _ = _hpx_step("munethpx_h16_8_norm")
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    _, ref, _, _ = _hpx_step("munethpx_h16_8_norm")
    for (name, a), (_, b) in zip(hip.named_parameters(), ref.named_parameters()):
        err = rel_l2(a.grad, b.grad)
        print(name, "%.2e" % err)
        assert err <= 1e-5, name
