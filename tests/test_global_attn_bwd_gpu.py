"""Backward of the diffusion U-Net's global attention on the GPU (dlwp_global_attn_bwd_f32 through
ops.global_attention_backward and training.global_attention): dq, dk and dv against fp64 autograd of the reference composition
(modern_unet.py:565-571) over token counts, head widths and batch sizes, bit determinism, batch independence and bad inputs."""
import pytest
import torch

from helpers import rel_l2

DEV = "cuda:0"


def _fp64_grad(qkv, grad_out, heads, d, scale):
    """autograd of einsum -> softmax over the queries -> einsum in float64, sample by sample: [Bt, N, heads 3 d]"""
    bt, n = qkv.shape[:2]
    out = torch.empty(qkv.shape, dtype=torch.float64, device=qkv.device)
    step = max(1, 2 ** 22 // (heads * n * n))
    for b0 in range(0, bt, step):
        x = qkv[b0:b0 + step].double().requires_grad_(True)
        q, k, v = x.reshape(x.shape[0], n, heads, 3, d).unbind(3)
        p = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) * scale, dim=2)
        o = torch.einsum("bhij,bjhd->bihd", p, v).reshape(x.shape[0], n, heads * d)
        out[b0:b0 + step], = torch.autograd.grad(o, x, grad_out[b0:b0 + step].double())
    return out


def _case(bt, n, heads, d, tag):
    from dlwp_benchmark_amd.weights import normal

    qkv = normal(f"gpu/gattn_bwd/{tag}/{bt}/{n}/{heads}/{d}/qkv", (bt, n, heads * 3 * d), 1.0).to(DEV) * 1.5
    go = normal(f"gpu/gattn_bwd/{tag}/{bt}/{n}/{heads}/{d}/go", (bt, n, heads * d), 1.0).to(DEV)
    return qkv, go


def _hip_grad(qkv, go, heads, d, scale=None):
    from dlwp_benchmark_amd import ops

    _, stats = ops.global_attention(qkv, heads, d, scale, return_stats=True)
    return ops.global_attention_backward(qkv, stats, go, heads, d, scale)


CASES = [
    # (Bt, N, heads, d)
    (1, 1, 1, 8),
    (2, 7, 2, 12),               # d = 12: not a multiple of 16
    (3, 16, 3, 16),
    (2, 129, 2, 64),             # tails of every tile
    (1, 1024, 4, 128),
    (1, 4096, 1, 64),
    (2, 35, 3, 13),              # d % 4 != 0: the element-wise load path
    (1, 129, 2, 256),            # d > 128: two output-column slices
    (1, 40, 1, 200),             # d > 128, not a multiple of 16
    (1, 64, 2, 1024),
    (1, 1024, 1, 1024),
    (4, 64, 4, 8),
]


@pytest.mark.gpu
@pytest.mark.parametrize("bt,n,heads,d", CASES)
def test_backward_matches_fp64_autograd(bt, n, heads, d):
    qkv, go = _case(bt, n, heads, d, "sweep")
    got = _hip_grad(qkv, go, heads, d).view(bt, n, heads, 3, d)
    want = _fp64_grad(qkv, go, heads, d, d ** -0.5).view(bt, n, heads, 3, d)
    if n == 1:
        # one query: every key's softmax weight is exactly 1, so dq = dk = 0 and only dv carries a gradient
        assert rel_l2(got[:, :, :, 2], want[:, :, :, 2]) <= 1e-5
        assert float(got[:, :, :, :2].abs().max()) <= 1e-6 * float(want[:, :, :, 2].abs().max())
        return
    errs = [rel_l2(got[:, :, :, t], want[:, :, :, t]) for t in range(3)]
    assert max(errs) <= 1e-5, f"rel L2 dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}"


@pytest.mark.gpu
def test_backward_batch_beyond_grid_y():
    """65538 samples of one head: more (sample, head) pairs than grid.y holds, so the host splits the batch"""
    bt, n, heads, d = 65538, 3, 1, 8
    qkv, go = _case(bt, n, heads, d, "gridy")
    got = _hip_grad(qkv, go, heads, d, 0.7).view(bt, n, heads, 3, d)
    want = _fp64_grad(qkv, go, heads, d, 0.7).view(bt, n, heads, 3, d)
    for t in range(3):
        assert rel_l2(got[:, :, :, t], want[:, :, :, t]) <= 1e-5
    tail = slice(65535 - 2, bt)
    assert rel_l2(got[tail], want[tail]) <= 1e-5


@pytest.mark.gpu
def test_backward_nside64_level0_pairs():
    """Bt = 96, N = 4096, 4 heads, d = 64 (the nside-64 level-0 shape at B = 8): a few (sample, head) pairs, the last one
    included (64-bit row bases)"""
    bt, n, heads, d = 96, 4096, 4, 64
    qkv, go = _case(bt, n, heads, d, "nside64")
    got = _hip_grad(qkv, go, heads, d).view(bt, n, heads, 3, d)
    for b in (0, 47, 95):
        want = _fp64_grad(qkv[b:b + 1], go[b:b + 1], heads, d, d ** -0.5).view(1, n, heads, 3, d)
        for h in (0, 3):
            err = rel_l2(got[b, :, h], want[0, :, h])
            assert err <= 1e-5, f"({b}, {h}): rel L2 {err:.2e}"


@pytest.mark.gpu
def test_autograd_function_uses_hip_and_matches_torch_recomputation(monkeypatch):
    from dlwp_benchmark_amd import training

    qkv, go = _case(2, 300, 2, 24, "fn")
    x = qkv.clone().requires_grad_(True)
    y = training.global_attention(x, 2, 24, 24 ** -0.5)
    y.backward(go)
    hip = x.grad.clone()
    assert torch.equal(hip, _hip_grad(qkv, go, 2, 24))
    monkeypatch.setenv("DLWP_TRAIN_TORCH_BACKWARD", "1")
    x.grad = None
    training.global_attention(x, 2, 24, 24 ** -0.5).backward(go)
    assert rel_l2(hip, x.grad) <= 2e-5


@pytest.mark.gpu
def test_unsupported_head_dim_takes_the_torch_recomputation():
    """head_dim above 1024: the kernel returns DLWP_ERR_UNSUPPORTED, the autograd function recomputes with torch"""
    from dlwp_benchmark_amd import lib, ops, training

    qkv, go = _case(1, 9, 1, 1040, "wide")
    _, stats = ops.global_attention(qkv, 1, 1040, return_stats=True)
    with pytest.raises(lib.DlwpError, match="status -2:"):
        ops.global_attention_backward(qkv, stats, go, 1, 1040)
    x = qkv.clone().requires_grad_(True)
    training.global_attention(x, 1, 1040, 1040 ** -0.5).backward(go)
    assert rel_l2(x.grad, _fp64_grad(qkv, go, 1, 1040, 1040 ** -0.5)) <= 1e-5


@pytest.mark.gpu
def test_backward_deterministic_and_batch_independent():
    qkv, go = _case(3, 777, 2, 40, "det")
    a = _hip_grad(qkv, go, 2, 40)
    b = _hip_grad(qkv, go, 2, 40)
    one = _hip_grad(qkv[1:2].clone(), go[1:2].clone(), 2, 40)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a[1:2], one)


@pytest.mark.gpu
def test_backward_5d_layout_round_trips():
    from dlwp_benchmark_amd import ops

    qkv, go = _case(2, 50, 3, 16, "5d")
    flat = _hip_grad(qkv, go, 3, 16)
    q5 = qkv.view(2, 50, 3, 3, 16)
    _, stats = ops.global_attention(q5, 3, 16, return_stats=True)
    g5 = ops.global_attention_backward(q5, stats, go, 3, 16)
    assert g5.shape == q5.shape and torch.equal(g5.reshape(flat.shape), flat)


@pytest.mark.gpu
def test_backward_bad_inputs_raise():
    from dlwp_benchmark_amd import lib, ops

    qkv, go = _case(1, 8, 4, 8, "bad")
    _, stats = ops.global_attention(qkv, 4, 8, return_stats=True)
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv.cpu(), stats, go, 4, 8)            # CPU tensors
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv, stats.cpu(), go, 4, 8)
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv, stats, go.cpu(), 4, 8)
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv, stats, go, 4, 7)                  # width is not heads * 3 * d_k
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv[0], stats, go, 4, 8)               # not [Bt, N, .]
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv, stats, go[:, :7], 4, 8)           # grad_out shape
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv, stats[:, :, :7], go, 4, 8)        # statistics of another shape
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv.double(), stats, go, 4, 8)         # not float32
    with pytest.raises(lib.DlwpError):
        ops.global_attention_backward(qkv, stats, go, 0, 8)
