"""The loss kernel of csrc/optim.hip (dlwp_mse_loss_f32) through ops.mse_loss / losses.CustomMSELoss against the expression of
the reference's scripts/losses.py:175-188, `mean(((target - input) ** 2) * weights)`, written out here in float64 on the same
fp32 inputs, and float64 autograd of it.

Bounds: the loss to 1e-6 relative (positive terms, double partials and a double finish); input.grad to the project's rel-L2
bound of 1e-5 and elementwise to 2 ulp (the kernel rounds 2 (x - t) w / N once from double)."""
import numpy as np
import pytest
import torch

from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import losses, ops
from dlwp_benchmark_amd import training as T
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_BOUND, GRAD_BOUND = 1e-6, 1e-5


def partials(n):
    return int(L.load().dlwp_mse_loss_partials(n))


def several_sweeps_size():
    """a flat size whose partial count is capped: every workgroup sums several sweeps"""
    n = 2048 * 4096 * 2 + 4099
    assert 0 < partials(n) < n / 64 and partials(n) == partials(10 * n)
    return n


# (shape, weight shape or None, weight dtype)
CASES = [((2, 1, 3, 8, 16), None, None), ((2, 1, 3, 8, 16), (8, 16), torch.float32), ((2, 1, 3, 8, 16), (8, 16), torch.float64),
         ((2, 3, 5, 7), None, None), ((2, 3, 5, 7), (5, 7), torch.float32), ((1, 1, 2, 12, 4, 4), (12, 4, 4), torch.float64),
         ((1, 1, 2, 12, 4, 4), (12, 4, 4), torch.float32), ((3 * 4096 + 5,), None, None), ("sweeps", None, None)]


def inputs(shape, wshape, wdtype, seed=0):
    if shape == "sweeps":
        shape = (several_sweeps_size(),)
    g = torch.Generator().manual_seed(77 + seed)
    x = torch.randn(*shape, generator=g)
    t = torch.randn(*shape, generator=g)
    w = None if wshape is None else torch.rand(*wshape, generator=g, dtype=torch.float64).to(wdtype)
    return x, t, w


def reference(x, t, w, upstream=1.0):
    """the reference expression and its autograd in float64: (loss, d (upstream * loss) / d input)"""
    x64 = x.double().requires_grad_(True)
    d = (t.double() - x64) ** 2
    if w is not None:
        d = d * w.double()
    loss = torch.mean(d)
    (upstream * loss).backward()
    return loss.detach(), x64.grad


def assert_ulp(got, want64, ulps):
    want32 = want64.float().numpy()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want64.numpy())
    assert np.all(err <= ulps * np.spacing(np.abs(want32)).astype(np.float64))


@pytest.mark.parametrize("shape,wshape,wdtype", CASES)
def test_loss_and_gradient_match_float64(shape, wshape, wdtype):
    x, t, w = inputs(shape, wshape, wdtype)
    want, want_grad = reference(x, t, w)
    xg = x.to(DEV).requires_grad_(True)
    crit = losses.CustomMSELoss(weights=w, weighted=w is not None)
    loss = crit(xg, t.to(DEV))
    assert loss.dim() == 0 and loss.is_cuda
    assert loss.dtype == (torch.float64 if wdtype == torch.float64 else torch.float32)    # the reference's promotion
    loss.backward()
    rel = abs(float(loss.detach()) - float(want)) / float(want)
    gerr = rel_l2(xg.grad.cpu(), want_grad)
    print(f"mse {shape} w={wshape} {wdtype}: loss {rel:.2e}, grad rel-L2 {gerr:.2e}")
    assert rel <= LOSS_BOUND
    assert xg.grad.dtype == torch.float32 and xg.grad.shape == x.shape
    assert gerr <= GRAD_BOUND
    assert_ulp(xg.grad, want_grad, 2)


def test_whole_numbers_give_the_float64_loss():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (3, 5, 4099), generator=g).float()
    t = torch.randint(-8, 9, (3, 5, 4099), generator=g).float()
    w = torch.randint(0, 4, (5, 4099), generator=g).double()
    for weight in (None, w, w.float()):
        want, _ = reference(x, t, weight)
        got = ops.mse_loss(x.to(DEV), t.to(DEV), None if weight is None else weight.to(DEV))
        assert float(got.double()) == float(want if weight is w else want.float())


def test_upstream_gradient_scales():
    x, t, w = inputs((2, 3, 5, 7), (5, 7), torch.float32)
    _, want_grad = reference(x, t, w, upstream=3.0)
    xg = x.to(DEV).requires_grad_(True)
    (3 * ops.mse_loss(xg, t.to(DEV), w.to(DEV))).backward()
    assert rel_l2(xg.grad.cpu(), want_grad) <= GRAD_BOUND
    assert_ulp(xg.grad, want_grad, 3)             # one more rounding: the product with the upstream scalar
    # a float64 loss under an upstream gradient
    x, t, w = inputs((2, 1, 3, 8, 16), (8, 16), torch.float64)
    _, want_grad = reference(x, t, w, upstream=-0.25)
    xg = x.to(DEV).requires_grad_(True)
    (-0.25 * ops.mse_loss(xg, t.to(DEV), w)).backward()
    assert_ulp(xg.grad, want_grad, 2)             # a power of two: exact


def test_no_gradient_buffer_without_requires_grad():
    x, t, w = inputs((2, 1, 3, 8, 16), (8, 16), torch.float32)
    x, t, w = x.to(DEV), t.to(DEV), w.to(DEV)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda v: saved.append(v) or v, lambda v: v):
        loss = ops.mse_loss(x, t, w)
    assert not saved and not loss.requires_grad
    loss2, grad = ops.mse_loss_forward(x, t, w, need_grad=False)
    assert grad is None and torch.equal(loss, loss2)
    ops.mse_loss(x, t, w)                                              # warm: the allocator has every block it needs
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
    ops.mse_loss(x, t, w)
    without = torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - before
    xg = x.clone().requires_grad_(True)
    before = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
    ops.mse_loss(xg, t, w)
    with_grad = torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - before
    assert without < x.numel() * 4 <= with_grad - without
    with torch.autograd.graph.saved_tensors_hooks(lambda v: saved.append(v) or v, lambda v: v):
        ops.mse_loss(x.clone().requires_grad_(True), t, w)
    assert len(saved) == 1 and saved[0].shape == x.shape


def test_torch_backward_switch_agrees(monkeypatch):
    x, t, w = inputs((2, 3, 5, 7), (5, 7), torch.float64)
    xg = x.to(DEV).requires_grad_(True)
    loss = losses.CustomMSELoss(weights=w, weighted=True)(xg, t.to(DEV))
    loss.backward()
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    monkeypatch.setattr(ops, "mse_loss_forward", lambda *a, **k: pytest.fail("the HIP loss under the torch switch"))
    xt = x.to(DEV).requires_grad_(True)
    ref = losses.CustomMSELoss(weights=w, weighted=True)(xt, t.to(DEV))
    ref.backward()
    assert ref.dtype == loss.dtype == torch.float64
    assert abs(float(ref.detach()) - float(loss.detach())) <= LOSS_BOUND * float(ref.detach())
    assert rel_l2(xg.grad, xt.grad) <= GRAD_BOUND


def test_reruns_are_bitwise_identical_and_unaligned_inputs_work():
    x, t, w = inputs((3 * 4096 + 5,), None, None)
    want, want_grad = reference(x[1:], t[1:], None)
    xd, td = x.to(DEV), t.to(DEV)
    a, ga = ops.mse_loss_forward(xd[1:], td[1:], None, need_grad=True)        # 4-byte aligned views
    b, gb = ops.mse_loss_forward(xd[1:], td[1:], None, need_grad=True)
    assert torch.equal(a, b) and torch.equal(ga, gb)
    assert abs(float(a) - float(want)) <= LOSS_BOUND * float(want)
    assert_ulp(ga, want_grad, 2)
    assert float(xd[0]) == float(x[0])


def test_refusals():
    x = torch.randn(2, 3, 4, device=DEV)
    with pytest.raises(L.DlwpError, match="shape"):
        ops.mse_loss(x, x[:1])
    with pytest.raises(L.DlwpError, match="broadcast"):
        ops.mse_loss(x, x, torch.ones(5, device=DEV))
    with pytest.raises(L.DlwpError, match="only the input"):
        ops.mse_loss(x, x.clone().requires_grad_(True))
