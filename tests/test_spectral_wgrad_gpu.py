"""Spectral weight gradient on the GPU (dlwp_spectral_conv2d_wgrad_f32, csrc/spectral_any.hip):

  * SpectralConv2d(ci, co, ...).train(): y, dL/dx, dL/dweights1, dL/dweights2 against gradients of the REAL reference
    class (tests/golden/spectral_wgrad_*.npz, tools/make_golden_spectral_grad.py), rectangular channel counts included;
  * the kernel against `training.spectral_weight_grad` (torch on the same device) at widths fixtures would be too large for;
  * the GPU path no longer calls the torch composition; results are bitwise repeatable and replay from a HIP graph;
  * FNO2DModule optimisation steps at widths 32 and 48 against the oracle module; TFNO2DModule gradients against the
    same module with the torch composition in place of the kernel.

Tolerances are the project's: 1e-5 relative L2 at op level, 1e-4 for a network step (tests/test_training_gpu.py).  Where a
kernel-vs-torch comparison with many summed samples misses 1e-5, both are measured against `spectral_weight_grad` in
double on the CPU and the kernel's error may be at most twice the torch composition's (two fp32 sums in different orders).
Measured on an MI355X, kernel vs torch on the device: 4.0e-7 (W = 100), 4.1e-7 (B = 70), 4.3e-7 (every 64 x 64 shape, B = 32):
no shape came near 1e-5, so no kernel / torch pair against double had to be recorded.
"""
import os
import sys

import pytest
import torch

from helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["c24x40_32x64_m8x6_b3", "c12x4_16x16_m4_b2", "c5x2_12x20_m3x11_b2", "c32_32x64_m8x6_b40"]


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_spectral_grad as tool
    finally:
        sys.path.pop(0)
    return tool


@pytest.mark.parametrize("tag", TAGS)
def test_spectral_conv2d_gradients_match_reference(tag):
    from dlwp_benchmark_amd.models import SpectralConv2d
    from oracle.restate.fno import spectral_conv2d_ref

    tool = _tool()
    ci, co, h, w, m1, m2, b = tool.CASES[tag]
    g = load_golden(f"spectral_wgrad_{tag}")
    x, w1, w2, r = tool.case_tensors(tag)
    assert tool.tensor_sha(x, w1, w2, r) == str(g["sha"])
    mod = SpectralConv2d(ci, co, m1, m2).to(DEV).train()
    with torch.no_grad():
        mod.weights1.copy_(w1)
        mod.weights2.copy_(w2)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg)
    (y * r.to(DEV)).sum().backward()
    figures = dict(gw1=rel_l2(mod.weights1.grad, torch.from_numpy(g["gw1"])),
                   gw2=rel_l2(mod.weights2.grad, torch.from_numpy(g["gw2"])),
                   gx_head=rel_l2(xg.grad[0, :4], torch.from_numpy(g["gx_head"])),
                   y_head=rel_l2(y[0, :4], torch.from_numpy(g["y_head"])))
    if "gx" in g.files:
        figures["gx"] = rel_l2(xg.grad, torch.from_numpy(g["gx"]))
        figures["y"] = rel_l2(y, torch.from_numpy(g["y"]))
    else:   # stored as norm + projection (file size): the whole tensor against the restatement the CPU test pins to them
        adj = lambda t: torch.view_as_real(torch.view_as_complex(t.contiguous()).conj().transpose(0, 1).contiguous())
        figures["gx"] = rel_l2(xg.grad, spectral_conv2d_ref(r, adj(w1), adj(w2)))
        figures["y"] = rel_l2(y, spectral_conv2d_ref(x, w1, w2))
        figures["gx_norm"] = abs(float(xg.grad.double().norm()) - float(g["gx_norm"])) / float(g["gx_norm"])
    print(tag, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < 1e-5, (k, v)


KERNEL_SHAPES = {   # ci, co, h, w, m1, m2, b
    "c16": (16, 16, 64, 64, 12, 12, 32), "c32": (32, 32, 64, 64, 12, 12, 32), "c64": (64, 64, 64, 64, 12, 12, 32),
    "c128": (128, 128, 64, 64, 12, 12, 32), "c256": (256, 256, 64, 64, 12, 12, 32),
    "c64x192": (64, 192, 64, 64, 12, 12, 32), "w100": (24, 24, 48, 100, 6, 9, 4), "b70": (32, 32, 32, 64, 8, 6, 70),
}


def _operator(ci, co, h, w, m1, m2):
    from dlwp_benchmark_amd import training as T

    rows, _ = T.pde_arena_rows(h, m1)
    return T.SpectralOperator(ci, h, w, rows, rows, m2, 1.0, 1.0 / float(h * w), DEV, out_channels=co), rows


@pytest.mark.parametrize("name", list(KERNEL_SHAPES))
def test_weight_gradient_kernel_matches_torch_composition(name):
    from dlwp_benchmark_amd import training as T

    ci, co, h, w, m1, m2, b = KERNEL_SHAPES[name]
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(b, ci, h, w, generator=gen)
    gy = torch.randn(b, co, h, w, generator=gen)
    op, rows = _operator(ci, co, h, w, m1, m2)
    got = op.backward_weight(x.to(DEV), gy.to(DEV))
    want = T.spectral_weight_grad(x.to(DEV), gy.to(DEV), rows, rows, m2, 1.0, 1.0 / float(h * w))
    assert got.shape == want.shape
    rel = rel_l2(got, want)
    print(f"{name}: kernel vs torch on the device {rel:.3e}")
    if rel > 1e-5:
        exact = T.spectral_weight_grad(x.double(), gy.double(), rows, rows, m2, 1.0, 1.0 / float(h * w))
        err_k, err_t = rel_l2(got, exact), rel_l2(want, exact)
        print(f"{name}: kernel vs double {err_k:.3e}, torch vs double {err_t:.3e}")
        assert err_k <= 2.0 * err_t, (rel, err_k, err_t)


def _no_torch_composition(monkeypatch):
    from dlwp_benchmark_amd import training as T

    def refuse(*a, **k):
        raise AssertionError("the GPU path called training.spectral_weight_grad")

    monkeypatch.setattr(T, "spectral_weight_grad", refuse)


def _fno_kw(hidden):
    return dict(n_modes=[8, 8], constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_channels=hidden,
                lifting_channels=64, projection_channels=64, n_layers=3, context_size=1)


def test_gpu_path_does_not_call_the_torch_composition(monkeypatch):
    from dlwp_benchmark_amd.models import FNO2DModule, SpectralConv2d
    from dlwp_benchmark_amd.synthetic import navier_stokes

    _no_torch_composition(monkeypatch)
    mod = SpectralConv2d(8, 8, 4, 4).to(DEV).train()
    x = torch.randn(2, 8, 16, 16, device=DEV, requires_grad=True)
    mod(x).square().sum().backward()
    assert mod.weights1.grad is not None and float(mod.weights1.grad.abs().sum()) > 0 and x.grad is not None
    net = FNO2DModule(**_fno_kw(32)).to(DEV).train()
    prog = navier_stokes(2, 3, 32, 64, channels=2, seed=3)[2].to(DEV)
    net(prognostic=prog).square().mean().backward()
    for w in net.fno.fno_blocks.convs.weight:
        grad = next(p.grad for p in w.parameters())
        assert grad is not None and float(grad.abs().sum()) > 0


def test_weight_gradient_is_bitwise_repeatable():
    ci, co, h, w, m1, m2, b = 24, 40, 32, 64, 8, 6, 37
    op, _ = _operator(ci, co, h, w, m1, m2)
    x, gy = torch.randn(b, ci, h, w, device=DEV), torch.randn(b, co, h, w, device=DEV)
    a = op.backward_weight(x, gy).clone()
    op.backward_weight(torch.randn_like(x), gy)       # the workspace is overwritten in between
    assert torch.equal(a, op.backward_weight(x, gy))


def test_forward_backward_records_into_a_graph_and_replays_to_the_same_bits():
    """torch.cuda.graph around forward + backward of one SpectralConv2d (the process keeps its default queue count)."""
    from dlwp_benchmark_amd.models import SpectralConv2d

    mod = SpectralConv2d(12, 20, 4, 5).to(DEV).train()
    x = torch.randn(3, 12, 16, 32, device=DEV, requires_grad=True)
    r = torch.randn(3, 20, 16, 32, device=DEV)

    def run():
        mod.zero_grad(set_to_none=True)
        x.grad = None
        (mod(x) * r).sum().backward()
        return x.grad, mod.weights1.grad, mod.weights2.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up: plans, tables and workspaces exist before the capture
        for _ in range(2):
            eager = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    graph.replay()
    torch.cuda.synchronize()
    for e, f, s in zip(eager, first, outs):
        assert float(e.abs().sum()) > 0
        assert torch.equal(e, f) and torch.equal(f, s)


@pytest.mark.parametrize("hidden", [32, 48])
def test_fno_training_step_matches_oracle_autograd(hidden):
    """the shape of tests/test_training_gpu.py::test_fno_training_step_matches_oracle_autograd, at the specialised
    width and at one only the width-generic kernels take"""
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.restate.fno import FNO2DModuleRef

    kw = _fno_kw(hidden)
    model = FNO2DModule(**kw)
    fill_state_dict(model, std_fn=lambda n, s: 0.85 / s[0] ** 0.5 if "convs.weight" in n else None, gain=0.85)
    ref = FNO2DModuleRef(**kw)
    ref.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    prog = navier_stokes(3, 4, 32, 64, channels=2, seed=11)[2]
    target = navier_stokes(3, 3, 32, 64, channels=2, seed=12)[2]

    def step(m, dev):
        m = m.to(dev).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        opt.zero_grad()
        out = m(prognostic=prog.to(dev))
        loss = torch.nn.functional.mse_loss(out, target.to(dev))
        loss.backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
        opt.step()
        with torch.no_grad():
            m.eval()
            after = m(prognostic=prog.to(dev)).cpu()
        return float(loss.detach()), grads, after

    loss_g, grads_g, after_g = step(model, DEV)
    loss_c, grads_c, after_c = step(ref, "cpu")
    assert abs(loss_g - loss_c) <= 1e-5 * abs(loss_c)
    assert set(grads_g) == set(grads_c)
    for k in grads_c:
        gg = torch.view_as_real(grads_g[k]) if grads_g[k].is_complex() else grads_g[k]
        gc = torch.view_as_real(grads_c[k]) if grads_c[k].is_complex() else grads_c[k]
        print(hidden, k, f"{rel_l2(gg, gc):.2e}")
        assert rel_l2(gg, gc) < 1e-4, k
    assert rel_l2(after_g, after_c) < 1e-4


def test_tfno_gradients_match_the_torch_composition(monkeypatch):
    """The oracle holds no Tucker restatement: the same module, once with the kernel and once with
    `spectral_weight_grad` in its place (torch differentiates the Tucker reconstruction in both)."""
    from dlwp_benchmark_amd import training as T
    from dlwp_benchmark_amd.models import TFNO2DModule
    from dlwp_benchmark_amd.synthetic import navier_stokes
    from dlwp_benchmark_amd.weights import fill_state_dict

    t = TFNO2DModule(rank=0.5, **_fno_kw(48))
    fill_state_dict(t, std_fn=lambda n, s: 0.3 if ("core" in n or "factor" in n) else None, gain=0.85)
    with torch.no_grad():
        for w in t.fno.fno_blocks.convs.weight:
            w.core.mul_(0.85 / 48 ** 0.5 / float(w.dense().abs().pow(2).mean().sqrt()))
    t = t.to(DEV).train()
    prog = navier_stokes(3, 4, 32, 64, channels=2, seed=11)[2].to(DEV)
    target = navier_stokes(3, 3, 32, 64, channels=2, seed=12)[2].to(DEV)

    def grads():
        t.zero_grad(set_to_none=True)
        torch.nn.functional.mse_loss(t(prognostic=prog), target).backward()
        return {k: p.grad.detach().clone() for k, p in t.named_parameters()}

    got = grads()
    monkeypatch.setattr(T.SpectralOperator, "backward_weight",
                        lambda self, x, gy: T.spectral_weight_grad(x.float(), gy.float(), self.rows_in, self.rows_out,
                                                                   self.n_cols, self.fwd_scale, self.inv_scale))
    want = grads()
    assert set(got) == set(want) and any("core" in k for k in got)
    for k in want:
        a = torch.view_as_real(got[k]) if got[k].is_complex() else got[k]
        b = torch.view_as_real(want[k]) if want[k].is_complex() else want[k]
        print(k, f"{rel_l2(a, b):.2e}")
        assert rel_l2(a, b) < 1e-5, k
