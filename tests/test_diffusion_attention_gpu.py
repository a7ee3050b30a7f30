"""Global attention of the diffusion U-Net's AttentionBlock on the GPU (dlwp_global_attn_f32 through ops.global_attention /
ops.attention_block, reference modern_unet.py:520-585): the block and the attention=True networks against outputs of the REAL
reference classes (tests/golden/diffattn_*.npz, tools/make_golden_diffusion_attention.py), the kernel against an fp64
restatement over token counts, head widths and batch sizes, and the proof that no N x N tensor is allocated."""
import json

import pytest
import torch

from helpers import load_golden, per_step_rel_l2, rel_l2

DEV = "cuda:0"
OPS = ["c8", "c32", "c64_l0", "c1024", "c48_dk16"]
NETS = ["diffmunet_h32_64", "diffmunethpx_h32_64", "diffmunet_h8_16"]


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


def _restated(qkv, heads, d, scale=None, pairs=None):
    """fp64 column-softmax attention, key chunk by key chunk (no N x N tensor of the whole problem): [Bt, N, heads d]"""
    bt, n = qkv.shape[:2]
    scale = d ** -0.5 if scale is None else scale
    x = qkv.reshape(bt, n, heads, 3, d)
    out = torch.zeros(bt, n, heads, d, dtype=torch.float64, device=qkv.device)
    for b, h in pairs or [(b, h) for b in range(bt) for h in range(heads)]:
        q, k, v = (x[b, :, h, t].double() for t in range(3))
        for j0 in range(0, n, 1024):
            s = (q @ k[j0:j0 + 1024].T) * scale                      # [N queries, keys of the chunk]
            p = torch.exp(s - torch.logsumexp(s, dim=0, keepdim=True))  # normalised over the queries
            out[b, :, h] += p @ v[j0:j0 + 1024]
    return out.reshape(bt, n, heads * d)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", OPS)
def test_attention_block_matches_reference_golden(tag):
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_by_spec

    g = load_golden(f"diffattn_op_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    assert sha == str(g["sha"])
    m = AttentionBlock(**json.loads(str(g["kwargs"])))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    x = _inputs(g)["x"].to(DEV)
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    want = torch.from_numpy(g["y"])
    assert y.shape == want.shape
    err = rel_l2(y, want)
    assert err <= 1e-5, f"{tag}: rel L2 {err:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", NETS)
def test_attention_network_rollout_matches_reference_golden(tag):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec
    from oracle.restate.ddpm import DDPMSchedulerRestated

    g = load_golden(f"diffattn_model_{tag}")
    case = json.loads(str(g["kwargs"]))
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=0.7)
    assert sha == str(g["sha"])
    model = getattr(M, case["cls"])(**case["kwargs"])
    model.load_state_dict(_with_aliases(model, sd), strict=True)
    model = model.to(DEV).eval()
    args = {k: v.to(DEV) for k, v in _inputs(g).items()}
    sched = DDPMSchedulerRestated(case["betas"], seed=case["scheduler_seed"])
    sched.set_timesteps(case["nsteps"])
    torch.manual_seed(case["seed"])
    got = model(constants=args.get("constants"), prescribed=args.get("prescribed"), prognostic=args["prognostic"],
                noise_scheduler=sched)
    torch.cuda.synchronize()
    want = torch.from_numpy(g["y"])
    assert got.shape == want.shape
    errs = per_step_rel_l2(got, want)
    assert max(errs) <= 1e-5, f"{tag}: per-step rel L2 {['%.2e' % e for e in errs]}"


KERNEL_CASES = [
    # (Bt, N, heads, d)
    (1, 1, 1, 8),
    (2, 17, 2, 24),
    (3, 35, 3, 13),              # d % 4 != 0: the element-wise load path
    (2, 1024, 4, 64),
    (1, 4096, 1, 256),
    (1, 32, 4, 1024),
    (2, 1024, 1, 1024),
    (1, 16200, 1, 64),           # 90 x 180
    (1, 17, 2, 200),             # d > 128, not a multiple of 16
]


@pytest.mark.gpu
@pytest.mark.parametrize("bt,n,heads,d", KERNEL_CASES)
def test_kernel_matches_fp64_restatement(bt, n, heads, d):
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.weights import normal

    qkv = normal(f"gpu/gattn/{bt}/{n}/{heads}/{d}", (bt, n, heads * 3 * d), 1.0).to(DEV)
    qkv[..., :] *= 1.5          # scores of a few units: a softmax far from uniform
    got = ops.global_attention(qkv, heads, d)
    want = _restated(qkv, heads, d)
    err = rel_l2(got, want)
    assert err <= 1e-5, f"rel L2 {err:.2e}"


@pytest.mark.gpu
def test_kernel_nside64_level0_batch():
    """Bt heads of the nside-64 level-0 shape (B = 8: Bt = 96, N = 4096, d = 64, 4 heads); a few (sample, head) pairs
    restated, including the last one (64-bit row bases)"""
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.weights import normal

    bt, n, heads, d = 96, 4096, 4, 64
    qkv = normal("gpu/gattn/nside64", (bt, n, heads * 3 * d), 1.0).to(DEV)
    got = ops.global_attention(qkv, heads, d)
    pairs = [(0, 0), (47, 2), (95, 3)]
    want = _restated(qkv, heads, d, pairs=pairs)
    for b, h in pairs:
        err = rel_l2(got[b, :, h * d:(h + 1) * d], want[b, :, h * d:(h + 1) * d])
        assert err <= 1e-5, f"({b}, {h}): rel L2 {err:.2e}"


@pytest.mark.gpu
def test_block_with_non_default_d_k_matches_restatement():
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_state_dict, normal

    m = AttentionBlock(32, n_heads=3, d_k=24)
    fill_state_dict(m)
    m = m.to(DEV)
    x = normal("gpu/gattn/block_dk", (2, 32, 9, 11), 1.0).to(DEV)
    with torch.no_grad():
        y = m(x)
        t = x.reshape(2, 32, 99).transpose(1, 2).double()
        qkv = t @ m.projection.weight.double().T + m.projection.bias.double()
        res = _restated(qkv, 3, 24)
        want = (res @ m.output.weight.double().T + m.output.bias.double() + t).transpose(1, 2).reshape(2, 32, 9, 11)
    assert rel_l2(y, want) <= 1e-5


@pytest.mark.gpu
def test_block_allocates_no_n_by_n_tensor():
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_state_dict, normal

    bt, c, h, w = 24, 64, 64, 64                  # N = 4096, d = 64, 4 heads
    m = AttentionBlock(c)
    fill_state_dict(m)
    m = m.to(DEV)
    x = normal("gpu/gattn/mem", (bt, c, h, w), 1.0).to(DEV)
    with torch.no_grad():
        m(x)                                       # packed weights, allocator warm
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = m(x)
        torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    n, heads, d = h * w, 4, c
    bound = 4 * (bt * n * heads * 3 * d + bt * n * heads * d + bt * heads * n) + 64 * 2 ** 20
    assert extra < bound, f"peak extra {extra / 2 ** 20:.0f} MiB >= {bound / 2 ** 20:.0f} MiB"
    assert extra < 4 * bt * heads * n * n // 8     # far below even an eighth of the N x N scores
    del y


@pytest.mark.gpu
def test_deterministic_and_batch_independent():
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.weights import normal

    qkv = normal("gpu/gattn/det", (3, 777, 2 * 3 * 40), 1.0).to(DEV)
    a = ops.global_attention(qkv, 2, 40)
    b = ops.global_attention(qkv, 2, 40)
    one = ops.global_attention(qkv[1:2].clone(), 2, 40)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a[1:2], one)


@pytest.mark.gpu
def test_bad_inputs_raise():
    from dlwp_benchmark_amd import lib, ops
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock

    good = torch.zeros(1, 8, 4 * 3 * 8, device=DEV)
    with pytest.raises(lib.DlwpError):
        ops.global_attention(good.cpu(), 4, 8)                     # CPU tensor
    with pytest.raises(lib.DlwpError):
        ops.global_attention(good, 4, 7)                           # width is not heads * 3 * d_k
    with pytest.raises(lib.DlwpError):
        ops.global_attention(good[0], 4, 8)                        # not [Bt, N, .]
    with pytest.raises(lib.DlwpError):
        ops.global_attention(torch.zeros(1, 0, 96, device=DEV), 4, 8)   # no tokens
    with pytest.raises(lib.DlwpError):
        ops.global_attention(good.double(), 4, 8)                  # not float32
    with pytest.raises(lib.DlwpError):
        ops.global_attention(good, 0, 8)
    m = AttentionBlock(8).to(DEV)
    with torch.no_grad():
        with pytest.raises(lib.DlwpError):
            m(torch.zeros(1, 8, 2, 2))                             # CPU input
        with pytest.raises(lib.DlwpError):
            m(torch.zeros(1, 6, 2, 2, device=DEV))                 # channels do not match
