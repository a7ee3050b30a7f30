"""LayerNorm backward on HIP (csrc/layernorm_bwd.hip, training._LayerNormFn) through ops.layer_norm under autograd, against
fp64 autograd of F.layer_norm on the CPU: the cases and the bound (relative L2 <= 1e-5) of tests/test_layernorm_bwd_cpu.py,
two sizes at which a lane group sweeps more than once, bit checks, gradient selection, error codes, and one training step
of the three token backbones with torch.nn.functional.layer_norm patched to raise."""
import pytest
import torch
import torch.nn.functional as F

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd import training as T
from helpers import rel_l2
from test_layernorm_bwd_cpu import BOUND, LN_CASES, ln_autograd, ln_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# more rows than partial sums: every lane group accumulates over several sweeps
SWEEP_CASES = [((70001,), 16), ((5000,), 2048)]


def hip_grads(x, gamma, beta, gy, eps, needs=(True, True, True)):
    xs = [t.float().to(DEV).requires_grad_(need) for t, need in zip((x, gamma, beta), needs)]
    y = ops.layer_norm(xs[0], xs[1], xs[2], eps)
    wrt = [t for t in xs if t.requires_grad]
    grads = iter(torch.autograd.grad(y, wrt, gy.float().to(DEV)))
    return y, [next(grads) if t.requires_grad else None for t in xs]


def check(lead, c, eps):
    x, gamma, beta, gy = ln_inputs(lead, c)
    want = ln_autograd(x, gamma, beta, gy, eps)
    _, got = hip_grads(x, gamma, beta, gy, eps)
    for name, w, t in zip(("dx", "dgamma", "dbeta"), want, got):
        err = rel_l2(t, w)
        print(f"layernorm {lead} C={c} eps={eps:g} {name}: {err:.2e}")
        assert t.shape == w.shape and err <= BOUND, name


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("lead,c", LN_CASES)
def test_gradients_match_fp64_autograd(lead, c, eps):
    check(lead, c, eps)


@pytest.mark.parametrize("lead,c", SWEEP_CASES)
def test_gradients_over_several_sweeps(lead, c):
    assert 0 < L.load().dlwp_layernorm_bwd_partials(lead[0], c) < lead[0]
    check(lead, c, 1e-5)


def test_whole_numbers_give_exact_dbeta():
    g = torch.Generator().manual_seed(5)
    rows, c = 1501, 68
    x = torch.randint(-4, 5, (rows, c), generator=g).double()
    gamma = torch.randint(1, 4, (c,), generator=g).double()
    gy = torch.randint(-3, 4, (rows, c), generator=g).double()
    _, (_, _, dbeta) = hip_grads(x, gamma, torch.zeros(c, dtype=torch.float64), gy, 1e-5)
    assert torch.equal(dbeta.cpu().double(), gy.sum(dim=0))


def test_training_forward_is_the_inference_forward_and_saves_x_and_gamma_only():
    x, gamma, beta, gy = (t.float().to(DEV) for t in ln_inputs((130,), 132))
    with torch.no_grad():
        want = ops.layer_norm(x, gamma, beta, 1e-5)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = ops.layer_norm(x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True), 1e-5)
    assert y.requires_grad and torch.equal(y, want)
    assert sum(t.numel() for t in saved) == x.numel() + 132


def test_backward_reruns_are_bitwise_identical():
    x, gamma, _, gy = (t.float().to(DEV) for t in ln_inputs((70001,), 16))
    first = ops.layernorm_backward(x, gamma, gy, 1e-5)
    again = ops.layernorm_backward(x, gamma, gy, 1e-5)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (True, True, True)])
def test_only_the_wanted_gradients_are_computed(needs, monkeypatch):
    asked = []
    real = ops.layernorm_backward

    def spy(x, weight, grad_out, eps, need_x, need_weight, need_bias):
        asked.append((need_x, need_weight, need_bias))
        out = real(x, weight, grad_out, eps, need_x, need_weight, need_bias)
        assert [t is not None for t in out] == [need_x, need_weight, need_bias]
        return out

    monkeypatch.setattr(ops, "layernorm_backward", spy)
    x, gamma, beta, gy = ln_inputs((19,), 132)
    want = ln_autograd(x, gamma, beta, gy, 1e-5)
    _, got = hip_grads(x, gamma, beta, gy, 1e-5, needs)
    assert asked == [needs]
    for w, t, need in zip(want, got, needs):
        assert (t is not None) == need
        if need:
            assert rel_l2(t, w) <= BOUND


def test_non_contiguous_grad_out():
    x, gamma, beta, gy = ln_inputs((33,), 68)
    want = ln_autograd(x, gamma, beta, gy, 1e-5)
    xs = [t.float().to(DEV).requires_grad_(True) for t in (x, gamma, beta)]
    gy_t = gy.float().to(DEV).t().contiguous().t()
    assert not gy_t.is_contiguous()
    got = torch.autograd.grad(ops.layer_norm(*xs, 1e-5), xs, gy_t)
    for w, t in zip(want, got):
        assert rel_l2(t, w) <= BOUND


def test_misaligned_x_takes_the_torch_form(monkeypatch):
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "0")
    statuses = []
    real = ops.layernorm_backward

    def spy(*a, **k):
        try:
            out = real(*a, **k)
        except L.DlwpError as e:
            statuses.append(e.status)
            raise
        statuses.append(0)
        return out

    monkeypatch.setattr(ops, "layernorm_backward", spy)
    x, gamma, beta, gy = ln_inputs((19,), 132)
    want = ln_autograd(x, gamma, beta, gy, 1e-5)
    _, aligned = hip_grads(x, gamma, beta, gy, 1e-5)
    store = torch.zeros(x.numel() + 1, device=DEV)
    xm = store[1:].view(x.shape)
    xm.copy_(x.float())
    assert xm.data_ptr() % 16 != 0 and xm.is_contiguous()
    xm.requires_grad_(True)
    params = [t.float().to(DEV).requires_grad_(True) for t in (gamma, beta)]
    got = torch.autograd.grad(ops.layer_norm(xm, *params, 1e-5), [xm, *params], gy.float().to(DEV))
    assert statuses == [0, L.ERR_UNSUPPORTED]
    for w, a, t in zip(want, aligned, got):
        assert rel_l2(t, w) <= BOUND and rel_l2(t, a) <= BOUND


def test_error_codes():
    """every call returns before a launch"""
    lib = L.load()
    rows, c = 8, 64
    x = torch.zeros(rows, 2052, device=DEV)
    gamma = torch.zeros(2052, device=DEV)
    out = torch.zeros(2052, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    need = int(lib.dlwp_layernorm_bwd_workspace_bytes(rows, c))
    assert need == 2 * lib.dlwp_layernorm_bwd_partials(rows, c) * c * 4 and 0 < need <= ws.numel()
    assert lib.dlwp_layernorm_bwd_workspace_bytes(rows, 6) == 0 and lib.dlwp_layernorm_bwd_partials(rows, 2052) == 0
    p = lambda t: t.data_ptr()
    call = lambda x_, g_, gy_, dx_, dg_, db_, ws_, nb, r, ch: lib.dlwp_layernorm_bwd_f32(
        x_, g_, gy_, dx_, dg_, db_, ws_, nb, r, ch, 1e-5, L.stream_ptr())
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    assert call(p(x), p(gamma), p(x), p(x), p(out), p(out), p(ws), ws.numel(), rows, 6) == UNSUPPORTED
    assert call(p(x), p(gamma), p(x), p(x), p(out), p(out), p(ws), ws.numel(), rows, 2052) == UNSUPPORTED
    assert call(p(x) + 4, p(gamma), p(x), p(x), p(out), p(out), p(ws), ws.numel(), rows, c) == UNSUPPORTED
    assert call(p(x), p(gamma), p(x), p(x), p(out), p(out), p(ws), need - 1, rows, c) == WORKSPACE
    assert call(None, p(gamma), p(x), p(x), p(out), p(out), p(ws), ws.numel(), rows, c) == INVALID
    assert call(p(x), None, p(x), p(x), p(out), p(out), p(ws), ws.numel(), rows, c) == INVALID
    assert call(p(x), p(gamma), None, p(x), p(out), p(out), p(ws), ws.numel(), rows, c) == INVALID
    assert call(p(x), p(gamma), p(x), p(x), p(out), None, None, 0, rows, c) == INVALID
    assert call(p(x), p(gamma), p(x), p(x), p(out), p(out), p(ws), ws.numel(), 0, c) == INVALID
    assert call(p(x), p(gamma), p(x), p(x), p(out), p(out), p(ws), ws.numel(), rows, 0) == INVALID
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(x.any())
    with pytest.raises(L.DlwpError) as e:
        ops.layernorm_backward(x[:, :6].contiguous(), gamma[:6].contiguous(), x[:, :6].contiguous(), 1e-5)
    assert e.value.status == L.ERR_UNSUPPORTED


def test_torch_backward_switch_agrees_with_the_kernel(monkeypatch):
    x, gamma, beta, gy = ln_inputs((130,), 260)
    _, hip = hip_grads(x, gamma, beta, gy, 1e-6)
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    monkeypatch.setattr(ops, "layernorm_backward", lambda *a, **k: pytest.fail("HIP backward under the torch switch"))
    _, ref = hip_grads(x, gamma, beta, gy, 1e-6)
    for a, b in zip(hip, ref):
        assert rel_l2(a, b) <= BOUND


# one training step of each token backbone without torch's layer_norm: tests/test_training_gpu.py's comparison with the
# gradients of the real reference classes (1e-4), run with spies on the new operators
@pytest.mark.parametrize("tag", ["swin_e32_32x64", "pangu_e48_32x64", "afno_e16_32x64"])
def test_training_step_runs_layernorm_and_linear_epilogue_on_hip(tag, monkeypatch):
    from test_training_gpu import test_training_gradients_match_reference as run_training_case

    def no_torch_layer_norm(*a, **k):
        raise AssertionError("torch.nn.functional.layer_norm called in a training step")

    monkeypatch.setattr(F, "layer_norm", no_torch_layer_norm)
    counts = {"ln": 0, "ln_bwd": 0, "lin": 0, "act": 0, "lin_bwd": 0}

    def counting(owner, name, key, when=lambda *a, **k: True):
        real = getattr(owner, name)

        def wrapper(*a, **k):
            counts[key] += bool(when(*a, **k))
            return real(*a, **k)

        monkeypatch.setattr(owner, name, wrapper)

    counting(T, "layer_norm", "ln")
    counting(ops, "layernorm_backward", "ln_bwd")
    # a Linear call the Function accepted (ops.linear asks _LinearFn.supported first) that has a bias or an activation
    counting(T, "linear_fn", "lin", when=lambda x, weight, bias, act=0, resid=None: bias is not None or act != 0)
    counting(T._ActFn, "apply", "act")      # the activation of a Linear whose GEMMs stay on torch: the same backward kernel
    counting(ops, "bias_act_backward", "lin_bwd")
    run_training_case(tag)
    print(tag, counts)
    assert counts["ln"] > 0 and counts["ln_bwd"] == counts["ln"]
    # (afno_e16: 16 input features, no Linear of it fits the GEMM kernel -- its GELUs still run on HIP)
    assert counts["lin"] + counts["act"] > 0 and counts["lin_bwd"] == counts["lin"] + counts["act"]
