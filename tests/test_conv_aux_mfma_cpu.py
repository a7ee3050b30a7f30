"""Host side of the matrix-pipe forms of the U-Net family's non-3x3 convolutions: every module whose forward calls ops.conv2d,
ops.conv_transpose2d or ops.small_module carries `aux_conv_form`, set_aux_conv_form and the constructor key reach it and
nothing else (`conv_form`, compute_precision and models without such modules stay as they were), and the C ABI of
csrc/conv_mfma.hip is in the ctypes table."""
import pytest
import torch

import dlwp_benchmark_amd.models as M
from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd import ops
from dlwp_benchmark_amd.models import diffusion as D
from dlwp_benchmark_amd.models import unet as U

UNET = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], n_convolutions=2)
MUNET = dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], norm=True)
DIFF = dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[8, 16], norm=True,
            num_refinement_step=2)
FAMILIES = [("UNet", UNET), ("UNetHPX", UNET), ("MUNetHPX", MUNET), ("ModernUNet", MUNET), ("DiffMUNetHPX", DIFF),
            ("DiffModernUNet", DIFF)]
# the module classes whose forward calls ops.conv2d / ops.conv_transpose2d / ops.small_module (directly or through _run_stack).
# ConvLSTM is not among them: its stacks hold only (pad, 3x3 convolution, activation) triples, which _run_stack fuses.
AUX_BEARING = (U.ResidualBlock, U._UNetEncoder, U._UNetDecoder, U._ModernUNetEncoder, U._ModernUNetDecoder,
               D.ResidualBlock, D.ModernUNetEncoder, D.ModernUNetDecoder)


def _aux(model):
    bearing = [m for m in model.modules() if isinstance(m, AUX_BEARING)]
    assert bearing, "no module with an auxiliary convolution found"
    for m in bearing:
        assert "aux_conv_form" in m.__dict__, type(m).__name__
    assert {id(m) for m in model.modules() if "aux_conv_form" in m.__dict__} == {id(m) for m in bearing}
    return {m.aux_conv_form for m in bearing}


def _conv(model):
    return [m.conv_form for m in model.modules() if "conv_form" in m.__dict__]


@pytest.mark.parametrize("name,cfg", FAMILIES)
def test_aux_conv_form_defaults_to_direct(name, cfg):
    assert _aux(getattr(M, name)(**cfg)) == {"direct"}


@pytest.mark.parametrize("name,cfg", FAMILIES)
def test_set_aux_conv_form(name, cfg):
    model = getattr(M, name)(**cfg)
    for form in ("bf16x6", "bf16", "direct"):
        assert model.set_aux_conv_form(form) is model
        assert _aux(model) == {form}
    model.set_aux_conv_form("bf16")
    with pytest.raises(L.DlwpError, match="nope"):
        model.set_aux_conv_form("nope")
    assert _aux(model) == {"bf16"}


@pytest.mark.parametrize("name,cfg", FAMILIES)
def test_the_two_conv_knobs_are_independent(name, cfg):
    model = getattr(M, name)(**cfg)
    before = _conv(model)
    model.set_aux_conv_form("bf16x6")
    assert _conv(model) == before and set(before) == {"direct"} and model.compute_precision == "fp32"
    model.set_conv_form("bf16")
    assert _aux(model) == {"bf16x6"}
    model.set_compute_precision("f16x3")
    assert _aux(model) == {"bf16x6"} and set(_conv(model)) == {"bf16x6"}
    model.set_compute_precision("fp32")
    assert _aux(model) == {"bf16x6"} and set(_conv(model)) == {"direct"}


@pytest.mark.parametrize("name,cfg", FAMILIES)
def test_constructor_key(name, cfg):
    model = getattr(M, name)(**cfg, aux_conv_form="bf16x6")
    assert _aux(model) == {"bf16x6"} and set(_conv(model)) == {"direct"}
    model = getattr(M, name)(**cfg, aux_conv_form="bf16", compute_precision="f16x3")
    assert _aux(model) == {"bf16"} and set(_conv(model)) == {"bf16x6"}
    with pytest.raises(L.DlwpError, match="nope"):
        getattr(M, name)(**cfg, aux_conv_form="nope")


def test_convlstm_has_no_auxiliary_convolution():
    model = M.ConvLSTM(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_sizes=[4, 4], height=8, width=16)
    assert not [m for m in model.modules() if hasattr(m, "aux_conv_form")]
    assert model.set_aux_conv_form("bf16x6") is model
    assert not [m for m in model.modules() if hasattr(m, "aux_conv_form")]


def test_set_aux_conv_form_drops_a_captured_step():
    model = M.UNet(**UNET)
    model._graphed = ("key", object())
    model.set_aux_conv_form("bf16x6")
    assert model._graphed is None
    model._graphed = ("key", object())
    with pytest.raises(L.DlwpError):
        model.set_aux_conv_form("nope")
    assert model._graphed is not None       # rejected before anything changed


def test_models_without_such_convolutions_are_untouched():
    model = M.SwinTransformer(constant_channels=1, prescribed_channels=0, prognostic_channels=1, context_size=1, img_height=8,
                              img_width=16, patch_size=2, embed_dim=8, depths=[2], num_heads=[2], window_size=2)
    before = {id(m): dict(m.__dict__) for m in model.modules()}
    model.set_aux_conv_form("bf16")
    assert not [m for m in model.modules() if hasattr(m, "aux_conv_form")]
    for m in model.modules():
        assert {k: v for k, v in m.__dict__.items() if k != "_graphed"} == \
            {k: v for k, v in before[id(m)].items() if k != "_graphed"}


def test_c_abi_is_in_the_ctypes_table():
    lib = L.load()
    for name in ("dlwp_conv2d_mfma_packed_bytes", "dlwp_conv2d_mfma_pack_f32", "dlwp_conv2d_mfma_f32",
                 "dlwp_conv_transpose2d_mfma_f32", "dlwp_conv2d_mfma_variant"):
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert len(L.SIGNATURES["dlwp_conv2d_mfma_f32"][1]) == len(L.SIGNATURES["dlwp_conv2d_f32"][1]) + 1
    assert len(L.SIGNATURES["dlwp_conv_transpose2d_mfma_f32"][1]) == len(L.SIGNATURES["dlwp_conv_transpose2d_f32"][1]) + 1


def test_packed_bytes():
    pb = L.load().dlwp_conv2d_mfma_packed_bytes
    # three bf16 images x k^2 taps x ceil(cin / 32) slabs x ceil(cout / 16) fragments x 1 KiB
    for cout, cin, k in ((1, 40, 1), (136, 272, 1), (136, 136, 3), (272, 272, 4), (8, 16, 2), (17, 33, 4)):
        assert pb(cout, cin, k) == 3 * k * k * ((cin + 31) // 32) * ((cout + 15) // 16) * 1024, (cout, cin, k)
    assert pb(0, 8, 1) == 0 and pb(8, -1, 1) == 0 and pb(8, 8, 0) == 0 and pb(8, 8, 5) == 0
    assert pb(1 << 20, 1 << 20, 1) == 0         # 2 GiB and more


def test_variant_query():
    """dlwp_conv2d_mfma_variant(transposed, batch, H, W, cout, k, stride, pad): 16 * fragment width + NF by the launchers' rule
    (live fragments of the GEMM pixel grid, then 512 workgroups; stride-2 convolutions have no NF = 1 instance)"""
    v = L.load().dlwp_conv2d_mfma_variant
    assert v(0, 0, 8, 8, 8, 1, 1, 0) == 0 and v(0, 1, 8, 8, 0, 1, 1, 0) == 0 and v(1, 1, 0, 8, 8, 4, 2, 1) == 0
    assert v(0, 1, 8, 8, 8, 3, 3, 1) == 0 and v(0, 1, 8, 8, 8, 5, 1, 2) == 0 and v(0, 1, 8, 8, 8, 3, 1, 3) == 0     # geometry
    assert v(1, 1, 8, 8, 8, 3, 2, 1) == 0 and v(1, 1, 8, 8, 8, 4, 2, 0) == 0 and v(1, 1, 8, 8, 8, 2, 1, 0) == 0
    assert v(0, 1, 2, 2, 8, 4, 1, 0) == 0                                           # empty output
    assert v(0, 384, 32, 32, 136, 1, 1, 0) == 16 * 16 + 4     # the 272 -> 136 shortcut: 8 tiles x 384 faces x 3 chunks
    assert v(0, 12, 8, 8, 6, 3, 2, 1) == 8 * 16 + 2           # 4 x 4 outputs: two rows of 8 lanes; NF 2 is the s = 2 minimum
    assert v(0, 384, 32, 32, 136, 3, 2, 1) == 16 * 16 + 4
    assert v(1, 384, 16, 16, 272, 4, 2, 1) == 16 * 16 + 4     # the 233 GFLOP up-sampling: 2 tiles x 384 x 2 parities x 5 chunks
    assert v(1, 12, 8, 8, 34, 4, 2, 1) == 8 * 16 + 1
    assert v(1, 1, 8, 16, 8, 2, 2, 0) == 16 * 16 + 1


def test_unknown_form_is_refused_before_any_tensor_check():
    x, w = torch.zeros(1, 3, 4, 4), torch.zeros(2, 3, 1, 1)
    with pytest.raises(L.DlwpError, match="unknown conv form"):
        ops.conv2d(x, w, None, form="fp32")
    with pytest.raises(L.DlwpError, match="unknown conv form"):
        ops.conv_transpose2d(x, torch.zeros(3, 2, 2, 2), None, 2, form="fp32")
    for m in (torch.nn.Conv2d(3, 2, 1), torch.nn.ConvTranspose2d(3, 2, 2, 2), torch.nn.AvgPool2d(2)):
        with pytest.raises(L.DlwpError, match="unknown conv form"):
            ops.small_module(m, x, form="fp32")
