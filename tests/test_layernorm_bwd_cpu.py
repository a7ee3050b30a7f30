"""The torch forms of the LayerNorm and Linear-epilogue backward kernels (training.layernorm_backward_torch,
training.bias_act_backward_torch: what csrc/layernorm_bwd.hip and csrc/bias_act.hip compute, term by term), in fp32 on the CPU
against fp64 autograd of F.layer_norm / F.gelu(F.linear(...)) + resid.

Bound: relative L2 <= 1e-5 for every gradient, the project's op-level bound (DESIGN sections 22-24).  Condition on the inputs:
for every case torch's OWN fp32 autograd must lie within 2.5e-6 of fp64 -- a case that does not (a row offset of 30 sigma at
C = 4 puts torch's fp32 backward at 8.5e-6) says nothing about the restated formula and does not belong here.  Rows have unit
variance and an offset of at most one sigma."""
import pytest
import torch
import torch.nn.functional as F

from dlwp_benchmark_amd import training as T
from helpers import rel_l2

BOUND = 1e-5
INPUT_CONDITION = 2.5e-6

# (leading shape, C): every (lanes per row, vectors per lane) instantiation of the kernel and its masked edge
LN_CASES = [((37,), 4), ((130,), 16), ((33,), 64), ((33,), 68), ((19,), 128), ((19,), 132), ((9,), 256), ((9,), 260),
            ((5,), 1028), ((3,), 2048), ((1,), 64), ((1,), 2048), ((2, 3, 7), 48)]


def ln_inputs(lead, c, seed=0, offset=True):
    g = torch.Generator().manual_seed(1000 * c + seed)
    x = torch.randn(*lead, c, generator=g, dtype=torch.float64)
    if offset:
        x = x + torch.randn(*lead, 1, generator=g, dtype=torch.float64)          # a row offset of about one sigma
    gamma = 1.0 + 0.5 * torch.randn(c, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(c, generator=g, dtype=torch.float64)
    gy = torch.randn(*lead, c, generator=g, dtype=torch.float64)
    return x, gamma, beta, gy


def ln_autograd(x, gamma, beta, gy, eps):
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    return torch.autograd.grad(F.layer_norm(x, (x.shape[-1],), gamma, beta, eps), (x, gamma, beta), gy)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("lead,c", LN_CASES)
def test_layernorm_backward_torch_matches_fp64_autograd(lead, c, eps):
    x, gamma, beta, gy = ln_inputs(lead, c)
    want = ln_autograd(x, gamma, beta, gy, eps)
    f32 = [t.float() for t in (x, gamma, beta, gy)]
    for name, w, t in zip(("dx", "dgamma", "dbeta"), want, ln_autograd(*f32, eps)):
        assert rel_l2(t, w) <= INPUT_CONDITION, f"{name}: torch's own fp32 backward is off on this input; replace the case"
    got = T.layernorm_backward_torch(f32[0], f32[1], f32[3], eps)
    for name, w, t in zip(("dx", "dgamma", "dbeta"), want, got):
        assert t.dtype == torch.float32 and t.shape == w.shape
        err = rel_l2(t, w)
        print(f"layernorm {lead} C={c} eps={eps:g} {name}: {err:.2e}")
        assert err <= BOUND, name


def test_layernorm_backward_torch_near_constant_gy():
    """a gradient that is almost the same in every channel: g - mean_C(g) cancels, the case the a term exists for.  (Rows
    without an offset and a tenth of the gradient varying: at 1 + 1e-2 noise on offset rows torch's own fp32 backward is
    1.1e-5 from fp64 and fails the input condition.)"""
    x, gamma, beta, gy = ln_inputs((130,), 64, seed=3, offset=False)
    gamma = torch.ones_like(gamma)
    gy = 1.0 + 0.1 * gy
    want = ln_autograd(x, gamma, beta, gy, 1e-5)
    f32 = [t.float() for t in (x, gamma, beta, gy)]
    for w, t in zip(want, ln_autograd(*f32, 1e-5)):
        assert rel_l2(t, w) <= INPUT_CONDITION
    for name, w, t in zip(("dx", "dgamma", "dbeta"), want, T.layernorm_backward_torch(f32[0], f32[1], f32[3], 1e-5)):
        assert rel_l2(t, w) <= BOUND, name


LINEAR_CASES = [(64, 32, 4), (96, 32, 128), (2048, 128, 32), (1, 32, 8)]


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rows,k,n", LINEAR_CASES)
def test_bias_act_backward_torch_matches_fp64_autograd(rows, k, n, act):
    g = torch.Generator().manual_seed(rows + 7 * n + act)
    x = torch.randn(rows, k, generator=g, dtype=torch.float64)
    w = torch.randn(n, k, generator=g, dtype=torch.float64) / k ** 0.5
    b = 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    resid = torch.randn(rows, n, generator=g, dtype=torch.float64)
    gy = torch.randn(rows, n, generator=g, dtype=torch.float64)

    def reference(x, w, b, resid, gy):
        b = b.detach().clone().requires_grad_(True)
        z = F.linear(x, w, b)
        z.retain_grad()
        y = (F.gelu(z) if act == 1 else z) + resid
        y.backward(gy)
        return z.detach(), z.grad, b.grad

    z, want_gz, want_db = reference(x, w, b, resid, gy)
    _, gz32, db32 = reference(*(t.float() for t in (x, w, b, resid, gy)))
    assert rel_l2(gz32, want_gz) <= INPUT_CONDITION and rel_l2(db32, want_db) <= INPUT_CONDITION
    gz, db = T.bias_act_backward_torch(gy.float(), z.float(), act)
    assert gz.dtype == torch.float32 and db.shape == (n,)
    print(f"bias_act rows={rows} n={n} act={act}: gz {rel_l2(gz, want_gz):.2e} db {rel_l2(db, want_db):.2e}")
    assert rel_l2(gz, want_gz) <= BOUND
    assert rel_l2(db, want_db) <= BOUND
