"""The diffusion U-Net with attention=True (reference modern_unet.py:46-121, :325-497, :520-585, :679-733): construction and
module layout of the mirror against what the REAL reference classes produced (tests/golden/diffattn_*.npz, written by
tools/make_golden_diffusion_attention.py).  No GPU needed."""
import json

import pytest
import torch
from torch import nn

from helpers import load_golden

NETS = ["diffmunet_h32_64", "diffmunethpx_h32_64", "diffmunet_h8_16"]
OPS = ["c8", "c32", "c64_l0", "c1024", "c48_dk16"]


def _net(tag):
    import dlwp_benchmark_amd.models as M

    g = load_golden(f"diffattn_model_{tag}")
    case = json.loads(str(g["kwargs"]))
    return getattr(M, case["cls"])(**case["kwargs"]), g


@pytest.mark.parametrize("cls", ["DiffModernUNet", "DiffMUNetHPX"])
def test_constructs_with_attention(cls):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock

    m = getattr(M, cls)(hidden_channels=[64, 128, 256, 1024], attention=True)
    blocks = [layer[-1] for layer in m.encoder.layers]
    assert all(isinstance(b, AttentionBlock) for b in blocks)
    assert [b.in_channels for b in blocks] == [64, 128, 256, 1024]
    assert all(b.n_heads == 4 and b.d_k == b.in_channels and b.scale == b.d_k ** -0.5 for b in blocks)
    assert blocks[-1].projection.out_features == 12 * 1024 and blocks[-1].output.in_features == 4 * 1024


@pytest.mark.parametrize("tag", NETS)
def test_state_dict_matches_reference(tag):
    m, g = _net(tag)
    want = [(k, s, d) for k, s, d in json.loads(str(g["state_spec"]))]
    got = [(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in m.state_dict().items()]
    assert got == want                                        # keys, shapes, dtypes AND order
    assert [[k, list(p.shape)] for k, p in m.named_parameters()] == json.loads(str(g["param_spec"]))


@pytest.mark.parametrize("tag", NETS)
def test_aliasing_and_identity_slots(tag):
    m, _ = _net(tag)
    enc = m.encoder
    assert enc.attn is enc.layers[-1][-1]
    assert list(enc._modules)[:2] == ["attn", "layers"]
    assert any(k.startswith("encoder.attn.") for k in m.state_dict())
    assert "encoder.layers.0.1.projection.weight" in m.state_dict()
    # the flag reaches the encoder only
    assert isinstance(m.middle.attn, nn.Identity)
    assert isinstance(m.decoder.attn, nn.Identity)
    assert all(not any(k.endswith("projection.weight") for k, _ in layer.named_parameters()) for layer in m.decoder.layers)


@pytest.mark.parametrize("tag", NETS)
def test_reference_state_dict_loads_strict(tag):
    from dlwp_benchmark_amd.weights import fill_by_spec

    m, g = _net(tag)
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=0.7)
    assert sha == str(g["sha"])
    # a reference-format state dict names the shared block twice
    last = len(m.encoder.layers) - 1
    slot = len(m.encoder.layers[last]) - 1
    for k in list(sd):
        if k.startswith("encoder.attn."):
            sd[f"encoder.layers.{last}.{slot}." + k[len("encoder.attn."):]] = sd[k]
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.encoder.layers[last][slot].projection.weight, sd["encoder.attn.projection.weight"])


def test_direct_middle_and_decoder_build_blocks():
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock, MiddleBlock, ModernUNetDecoder

    mid = MiddleBlock(in_channels=32, time_embed_dim=64, attention=True)
    assert isinstance(mid.attn, AttentionBlock) and mid.attn.in_channels == 32
    assert list(mid._modules) == ["res1", "attn", "res2"]
    dec = ModernUNetDecoder(hidden_channels=[16, 32], out_channels=2, time_embed_dim=64, attention=True)
    assert [layer[1].in_channels for layer in dec.layers] == [32, 16]
    assert dec.attn is dec.layers[-1][1]
    keys = list(dec.state_dict())
    assert keys.index("attn.projection.weight") < keys.index("layers.0.0.conv1.weight")
    assert not isinstance(MiddleBlock(in_channels=8, time_embed_dim=16).attn, AttentionBlock)


@pytest.mark.parametrize("tag", OPS)
def test_attention_block_layout_matches_reference(tag):
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock

    g = load_golden(f"diffattn_op_{tag}")
    m = AttentionBlock(**json.loads(str(g["kwargs"])))
    got = [(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in m.state_dict().items()]
    assert got == [(k, s, d) for k, s, d in json.loads(str(g["state_spec"]))]


def test_attention_block_cpu_tensor_raises():
    from dlwp_benchmark_amd import lib
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock

    m = AttentionBlock(8)
    with torch.no_grad(), pytest.raises(lib.DlwpError):
        m(torch.zeros(1, 8, 2, 2))


def test_attention_block_grad_path_matches_fp64_restatement():
    """with gradients wanted the block runs torch operators: the reference arithmetic, checked against an fp64 restatement"""
    from dlwp_benchmark_amd.models.diffusion import AttentionBlock
    from dlwp_benchmark_amd.weights import fill_state_dict, normal

    m = AttentionBlock(12, d_k=5)
    fill_state_dict(m)
    x = normal("cpu/attnblock/x", (2, 12, 3, 5)).requires_grad_(True)
    y = m(x)
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    want = _restated(x.detach().double(), m, 4, 5)
    assert torch.allclose(y.detach().double(), want, rtol=1e-5, atol=1e-5)


def _restated(x, m, heads, d):
    b, c, h, w = x.shape
    n = h * w
    t = x.reshape(b, c, n).transpose(1, 2)
    qkv = t @ m.projection.weight.double().T + m.projection.bias.double()
    qkv = qkv.reshape(b, n, heads, 3, d)
    q, k, v = qkv[..., 0, :], qkv[..., 1, :], qkv[..., 2, :]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * d ** -0.5
    p = torch.exp(s - torch.logsumexp(s, dim=2, keepdim=True))          # normalised over the queries i
    res = torch.einsum("bhij,bjhd->bihd", p, v).reshape(b, n, heads * d)
    y = res @ m.output.weight.double().T + m.output.bias.double() + t
    return y.transpose(1, 2).reshape(b, c, h, w)
